"""Seed mode from HBM: serve a model's xorbs to BitTorrent (BEP XET) peers straight out of GPU memory.

`HbmXorbArena` serializes every xorb of a model (8-byte chunk headers + payloads, the CAS wire
form) into one device buffer with the GPU pack kernel (K7); `HbmSeedServer` registers each xorb's
chunk boundaries with the native `_hip.HbmSeeder`, whose provider copies requested chunk runs
HBM → pinned host → socket with no intermediate host copy.  This is the MI355X counterpart of the
reference's disk-backed seeding (src/server.zig:187-215) sized for 288 GB of HBM per GPU
(BASELINE config: "Mixtral-8x7B seed mode: serve xorbs from 288 GB HBM, measure chunks_served/s").

`ResidentSeedServer` needs no serialized copy: it serves the xorbs of files that are resident in HBM
as decoded bytes (a device pull's buffers, `pull(..., device="cuda:N", seed=True)`), re-serializing
each requested chunk range on the GPU (`ops.serve_pack`, csrc/gpu/serve.hip) from a table built by
`plan_resident_runs`.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _core, ops
from .synthetic import SyntheticWorld


class HbmXorbArena:
    def __init__(self, world: SyntheticWorld, content: torch.Tensor, device=None, batch_chunks: int = 1 << 20):
        if world.terms is None:
            raise ValueError("world must be built (build_on_device / build_on_host) first")
        self.world = world
        dev = torch.device(device) if device is not None else content.device
        ser = world.chunk_clen.astype(np.uint64) + np.uint64(8)  # stored size (BG4-LZ4 frames in bf16 worlds)
        out_off = (np.cumsum(ser) - ser).astype(np.uint64)
        self.nbytes = int(ser.sum())
        self.buf = ops.padded_empty(self.nbytes, dev)
        for a in range(0, world.n_chunks, batch_chunks):
            b = min(world.n_chunks, a + batch_chunks)
            world.pack_serialized(content, a, b, self.buf, out_off[a:b])
        x0 = world.xorb_chunk0
        x1 = np.concatenate([x0[1:], [world.n_chunks]])
        self.xorb_off = out_off[x0]
        cum = np.cumsum(ser)
        self.xorb_ends = [(cum[a:b] - (cum[a] - ser[a])).astype(np.uint64) for a, b in zip(x0, x1)]
        # xorb hashes on the GPU (Merkle over each xorb's chunk hashes, K2)
        hashes = torch.from_numpy(np.ascontiguousarray(world.chunk_hashes)).to(dev)
        sizes = torch.from_numpy(world.chunk_len.astype(np.int64)).to(dev)
        roots = ops.merkle_roots(hashes, sizes, [(int(a), int(b - a)) for a, b in zip(x0, x1)], file_hash=False)
        self.xorb_hashes = [bytes(r) for r in roots.cpu().numpy()]
        self.xorb_hex = [_core.xet_hex(h) for h in self.xorb_hashes]
        torch.cuda.synchronize(dev) if dev.type == "cuda" else None


class HbmSeedServer:
    """BEP XET listener backed by an HbmXorbArena (optionally falling back to the disk cache)."""

    def __init__(self, arena: HbmXorbArena, port: int = 0, disk_fallback: bool = False):
        from . import ops as _ops
        H = _ops.hip()
        dev = arena.buf.device
        self.arena = arena
        self.seeder = H.HbmSeeder(arena.buf.data_ptr(), arena.nbytes, dev.index or 0, port, disk_fallback)
        for hx, off, ends in zip(arena.xorb_hex, arena.xorb_off, arena.xorb_ends):
            self.seeder.add_xorb(hx, int(off), ends.tolist())
        self.seeder.start()

    @property
    def port(self) -> int:
        return self.seeder.port

    def stats(self) -> dict:
        return self.seeder.stats()

    def stop(self) -> None:
        self.seeder.stop()


class HbmCacheArena:
    """Warm seeding: every run of the local xorb disk cache (`{hex}` / `{hex}.{chunk_offset}`)
    uploaded once into one HBM buffer (restore the arena from the disk cache at serve
    start)."""

    def __init__(self, device="cuda:0", max_bytes: int | None = None):
        import json
        import os

        import numpy as np

        cfg = json.loads(_core.config_json())
        root = cfg["xorb_cache_dir"]
        runs = []
        total = 0
        for pfx in sorted(os.listdir(root)) if os.path.isdir(root) else []:
            d = os.path.join(root, pfx)
            if len(pfx) != 2 or not os.path.isdir(d):
                continue
            for name in sorted(os.listdir(d)):
                hx, _, off = name.partition(".")
                if len(hx) != 64 or (off and not off.isdigit()):
                    continue
                path = os.path.join(d, name)
                size = os.path.getsize(path)
                if max_bytes is not None and total + size > max_bytes:
                    break
                runs.append((hx, int(off or 0), path, size))
                total += size
        dev = torch.device(device)
        self.nbytes = total
        self.buf = ops.padded_empty(max(total, 1), dev)
        self.runs = []  # (hex, dev_off, chunk_ends, first_chunk)
        pos = 0
        for hx, first, path, size in runs:
            data = np.fromfile(path, dtype=np.uint8)
            try:
                idx = _core.index_chunks(data)
            except Exception:
                continue  # not a chunk run (corrupt file): skip
            if not idx:
                continue
            ends = [e[0] + 8 + e[1] for e in idx]
            n = ends[-1]
            self.buf[pos:pos + n].copy_(torch.from_numpy(data[:n]), non_blocking=False)
            self.runs.append((hx, pos, ends, first))
            pos += n
        self.used = pos


class HbmCacheSeedServer:
    """BEP XET seeder over an HbmCacheArena (falls back to the disk cache for anything else)."""

    def __init__(self, arena: HbmCacheArena, port: int = 0):
        H = ops.hip()
        dev = arena.buf.device
        self.arena = arena
        self.seeder = H.HbmSeeder(arena.buf.data_ptr(), max(arena.used, 1), dev.index or 0, port, True)
        for hx, off, ends, first in arena.runs:
            self.seeder.add_xorb(hx, int(off), ends, int(first))
        self.seeder.start()

    @property
    def port(self) -> int:
        return self.seeder.port

    def stats(self) -> dict:
        return self.seeder.stats()

    def stop(self) -> None:
        self.seeder.stop()


def merge_chunk_refs(refs: dict) -> dict:
    """`{xorb_hex: [(first_chunk, addrs, lens), ...]}` with overlapping or neighbouring references
    -> the same map with maximal runs of consecutive chunk indices, sorted by first_chunk; a chunk
    index referenced more than once keeps its first reference.  The merge step of
    plan_resident_runs, also used to unite two plans (zest_amd.delta.ResidentSet)."""
    plan = {}
    for hx, rs in refs.items():
        idx = np.concatenate([np.arange(c0, c0 + len(a), dtype=np.int64) for c0, a, _ in rs])
        addrs = np.concatenate([a for _, a, _ in rs])
        lens = np.concatenate([ln for _, _, ln in rs])
        idx, first = np.unique(idx, return_index=True)  # sorted indices, first reference of each
        addrs, lens = addrs[first], lens[first]
        cuts = np.flatnonzero(np.diff(idx) != 1) + 1
        plan[hx] = [(int(i[0]), a, ln) for i, a, ln in
                    zip(np.split(idx, cuts), np.split(addrs, cuts), np.split(lens, cuts))]
    return plan


def plan_resident_runs(files) -> dict:
    """Where every xorb chunk of a set of decoded files sits in memory.

    files: per file `(ptr, chunk_lens, term_keys)` -- the address of its decoded bytes, its chunk
    sizes in file order (uint32 array or little-endian bytes, `DeviceXetPull.pull_files`'s
    `chunk_lens`) and its reconstruction terms `[(xorb_hex, chunk_start, chunk_end), ...]`
    (`DeviceXetPull.term_keys`).  Walks the terms with a running chunk cursor and merges them, across
    terms and files, into maximal runs of consecutive xorb chunk indices (another file's fetch range
    may span two terms of this one); a chunk index referenced more than once keeps its first
    reference.  Returns `{xorb_hex: [(first_chunk, addrs, lens), ...]}` (uint64 / uint32 arrays), runs
    sorted by first_chunk.  A file whose terms do not account for exactly its chunks raises."""
    refs: dict[str, list] = {}
    for fi, (ptr, chunk_lens, terms) in enumerate(files):
        lens = (np.frombuffer(chunk_lens, dtype="<u4") if isinstance(chunk_lens, (bytes, bytearray, memoryview))
                else np.asarray(chunk_lens)).astype(np.uint32)
        offs = np.uint64(int(ptr)) + (np.cumsum(lens, dtype=np.uint64) - lens)
        cur = 0
        for ti, (hx, c0, c1) in enumerate(terms):
            k = int(c1) - int(c0)
            if k <= 0 or cur + k > len(lens):
                raise ValueError(f"file {fi} term {ti}: chunks [{c0}, {c1}) of {hx} do not match the file's "
                                 f"{len(lens)} chunks (cursor {cur})")
            refs.setdefault(hx, []).append((int(c0), offs[cur:cur + k], lens[cur:cur + k]))
            cur += k
        if cur != len(lens):
            raise ValueError(f"file {fi}: terms cover {cur} chunks, chunk_lens has {len(lens)}")
    return merge_chunk_refs(refs)


_active: list = []  # ResidentSeedServers started by pull(..., seed=...)


def active() -> list:
    """The resident seed servers started by `pull(..., seed=...)` that are still running."""
    return list(_active)


def stop_all() -> None:
    for srv in list(_active):
        srv.stop()


class ResidentSeedServer:
    """BEP XET seeder over files that are resident in HBM as decoded bytes (a device pull's buffers).

    files: per file `(buffer, chunk_lens, term_keys)` with `buffer` a uint8 device tensor holding the
    whole file (see plan_resident_runs for the other two).  A requested chunk range is serialized on
    the GPU from those bytes straight into the connection's pinned staging buffer (`_hip.HbmSeeder`
    resident runs, csrc/gpu/serve.hip): HBM holds no second, serialized copy of the model, only one
    table of 16 bytes per chunk, and no disk is involved.

    The server keeps the buffers and the table alive until stop().  It is meant for read-only
    weights: bytes changed in place no longer match their chunk hashes, and receivers drop them."""

    def __init__(self, files, device="cuda:0", port: int = 0):
        files = [(b, lens, list(keys)) for b, lens, keys in files]
        plan = plan_resident_runs([(b.data_ptr(), lens, keys) for b, lens, keys in files])
        self._start(plan, [b for b, _, _ in files], device, port)

    @classmethod
    def from_plan(cls, plan: dict, buffers, device="cuda:0", port: int = 0) -> "ResidentSeedServer":
        """Serve a ready plan `{xorb_hex: [(first_chunk, addrs, lens), ...]}` whose chunks lie in
        `buffers` (uint8 device tensors)."""
        self = cls.__new__(cls)
        self._start(plan, list(buffers), device, port)
        return self

    def _start(self, plan: dict, buffers: list, device, port: int) -> None:
        H = ops.hip()
        dev = torch.device(device)
        if dev.type != "cuda":
            raise ValueError("ResidentSeedServer serves from GPU memory")
        for b in buffers:
            if b.device != dev or b.dtype != torch.uint8 or not b.is_contiguous():
                raise ValueError("file buffers must be contiguous uint8 tensors on the serving device")
        self.plan = plan
        self.buffers = buffers
        runs = [(hx, first, addrs, lens) for hx, rs in plan.items() for first, addrs, lens in rs]
        n = sum(len(a) for _, _, a, _ in runs)
        ends = [np.cumsum(np.asarray(ln).astype(np.uint64) + np.uint64(8), dtype=np.uint64) for _, _, _, ln in runs]
        tab = (np.concatenate([np.asarray(a, dtype=np.uint64) for _, _, a, _ in runs] + ends) if runs
               else np.zeros(0, np.uint64))
        self.table = torch.from_numpy(tab.view(np.int64).copy()).to(dev)  # [addresses | serialized ends]
        self.table_bytes = 16 * n
        torch.cuda.synchronize(dev)
        self.seeder = H.HbmSeeder(0, 0, dev.index or 0, port, False)
        for b in self.buffers:
            self.seeder.add_resident_buffer(b.data_ptr(), b.numel())
        at = 0
        for (hx, first, addrs, _), e in zip(runs, ends):
            self.seeder.add_resident_run(hx, first, self.table.data_ptr() + 8 * at,
                                         self.table.data_ptr() + 8 * (n + at), e.tolist())
            at += len(addrs)
        self.xorbs = sorted(plan)
        self.seeder.start()

    @property
    def port(self) -> int:
        return self.seeder.port

    def stats(self) -> dict:
        return self.seeder.stats() if self.seeder is not None else self._last_stats

    def stop(self) -> None:
        """Stop serving, then let go of the file buffers and the table."""
        if self.seeder is None:
            return
        self._last_stats = self.seeder.stats()
        self.seeder.stop()
        if self in _active:
            _active.remove(self)
        self.seeder = None  # joins the connection threads before the memory they read is released
        self.buffers = []
        self.table = None


def seed_port(seed) -> int | None:
    """The port a `seed=` keyword asks for: None when off, 0 for an OS-chosen one."""
    if seed is None or seed is False:
        return None
    if seed is True:
        return 0
    if isinstance(seed, int) and 0 <= seed < 65536:
        return int(seed)
    raise ValueError("seed= takes False, True (OS-chosen port) or a port number")


def main(argv=None) -> int:
    """`python -m zest_amd.seed [--port P] [--device cuda:0] [--max-gb G]`: seed the local xorb cache
    from HBM until interrupted.  With `--pull REPO [--revision R]`: pull the repo's weights into HBM
    (no disk) and seed them from there."""
    import argparse
    import signal
    import threading

    ap = argparse.ArgumentParser(description="seed the local xorb cache (or a fresh device pull) from GPU memory")
    ap.add_argument("--port", type=int, default=6881)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--max-gb", "--hbm-cache-gb", dest="max_gb", type=float, default=None)
    ap.add_argument("--pull", metavar="REPO", default=None, help="pull REPO into HBM and seed its resident weights")
    ap.add_argument("--revision", default="main")
    a = ap.parse_args(argv)
    if a.pull:
        from .direct import pull_to_device

        weights = pull_to_device(a.pull, a.revision, a.device, seed=a.port)
        srvs = active()
        if not srvs:
            print(f"{a.pull}@{a.revision} has no Xet-backed safetensors files: nothing to seed", flush=True)
            return 1
        srv = srvs[-1]
        print(f"HBM seeder: {len(srv.xorbs)} xorbs resident as {len(weights)} tensors on {a.device} "
              f"(+{srv.table_bytes / 1e6:.2f} MB of tables), BT listen port {srv.port}", flush=True)
    else:
        arena = HbmCacheArena(a.device, None if a.max_gb is None else int(a.max_gb * 1e9))
        srv = HbmCacheSeedServer(arena, a.port)
        print(f"HBM seeder: {len(arena.runs)} cached runs, {arena.used / 1e9:.2f} GB on {a.device}, "
              f"BT listen port {srv.port}", flush=True)
    stop = threading.Event()
    signal.signal(signal.SIGINT, lambda *_: stop.set())
    signal.signal(signal.SIGTERM, lambda *_: stop.set())
    stop.wait()
    srv.stop()
    print("stats:", srv.stats(), flush=True)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
