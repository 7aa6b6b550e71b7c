"""Collective sharded pull: `pull(repo, device="all", shard=...)`.  Within one process group every
safetensors file is fetched and Xet-verified by exactly one rank, its owner, and every rank takes
only its own slices of it out of the owner's memory.  Network bytes per node drop by `world`; each
rank holds its kept slices plus one scratch.

A plain collective in synchronous rounds, as swarm_load: no elastic membership, no streamed
agreement, no signal pages.  A rank that fails makes every rank raise.

Plan.  Rank 0 lists the repository (and reads model.safetensors.index.json) and broadcasts both.  A
file is skipped only when no rank keeps anything of it.  Owners are assigned by size
(swarm_load.assign_owners); each owner cuts its files into groups that fit its scratch
(direct._groups).  Round j is every rank's j-th group; a rank may have none.

Round.  The owner pulls its group whole into its scratch (a Xet file hash can only be checked over
the whole file: DeviceXetPull.pull_files / HostXetFetcher.fetch_files, file hash check and CDN
repair as in the single-process pull) and synchronises its device; all ranks agree on success in
one all-reduce; the owners share their files' safetensors headers; every rank plans its slices
(shard.plan_file) and the slices are exchanged:

  "mapped"  (GPU) the scratch is an ops.vmm_empty arena that every peer maps once per pull
            (exchange.map_peer_arenas).  A rank gathers its slices of all the round's files with one
            ops.slice_gather_peers launch (K11) out of the owners' scratches into one compact arena.
            A second agreement, after every rank's gather has synchronised, lets the owners
            overwrite their scratches.
  "send"    (any backend, and the CPU path) the owner gathers every destination's slices into a send
            buffer with ops.slice_gather (K10) and the parts move with all_to_all_single, or with
            batch_isend_irecv where the backend has no all-to-all.  What a rank receives of a file is
            exactly its own plan_file arena.

What is verified: every file, whole, by its owner, against its Xet file hash.  A slice has no hash a
receiver could check; `cross_check=True` runs both paths every round and compares every kept byte.
"""
from __future__ import annotations

import contextlib
import os
import struct
import time

import numpy as np
import torch
import torch.distributed as dist

from .. import _core, ops
from .. import device as zdev
from .. import direct
from .. import shard as zshard
from . import exchange as zx
from .swarm_load import assign_owners

EXCHANGES = ("auto", "mapped", "send")


class ShardPullError(RuntimeError):
    """A rank of the collective sharded pull failed; raised on every rank."""


def _align(n: int) -> int:
    return -(-n // zshard.ARENA_ALIGN) * zshard.ARENA_ALIGN


class _Ctl:
    """Control traffic of one pull: object collectives and all-reduces over `group`.  gloo carries
    host tensors; any other backend (RCCL) gets tensors on the rank's device."""

    def __init__(self, group, device: torch.device):
        self.group = group
        self.rank, self.world = dist.get_rank(group), dist.get_world_size(group)
        self.backend = str(dist.get_backend(group)).lower()
        self.dev = torch.device("cpu") if self.backend == "gloo" else device
        self.global_ranks = dist.get_process_group_ranks(group) if group is not None else list(range(self.world))

    def failed(self, bad: bool) -> list[int]:
        """One all-reduce: the ranks on which `bad` is set."""
        flag = torch.zeros(self.world, dtype=torch.int32, device=self.dev)
        if bad:
            flag[self.rank] = 1
        dist.all_reduce(flag, op=dist.ReduceOp.MAX, group=self.group)
        return [r for r, v in enumerate(flag.tolist()) if v]

    def gather(self, obj) -> list:
        out = [None] * self.world
        dist.all_gather_object(out, obj, group=self.group)
        return out

    def from0(self, obj):
        box = [obj]
        dist.broadcast_object_list(box, src=self.global_ranks[0], group=self.group)
        return box[0]


def _listing(ctl: _Ctl, repo, revision, repo_type, net, include):
    """(files, index bytes or None) as rank 0 sees the repository, on every rank."""
    got = None
    if ctl.rank == 0:
        try:
            _, files = _core.list_repo_files(repo, revision, repo_type)
            index = None
            if any(f["path"] == zshard.INDEX_NAME for f in files):
                r = _core.pull(repo, revision, *net, [zshard.INDEX_NAME], True, 0, repo_type)
                with open(os.path.join(r["snapshot_dir"], zshard.INDEX_NAME), "rb") as fh:
                    index = fh.read()
            got = ("ok", [dict(f) for f in files], index)
        except Exception as e:  # noqa: BLE001  (told to every rank, re-raised here)
            got = ("error", f"{type(e).__name__}: {e}", e)
    res = ctl.from0(got if got is None or got[0] == "ok" else got[:2])
    if res[0] != "ok":
        if ctl.rank == 0:
            raise got[2]
        raise ShardPullError(f"rank 0 could not list {repo}: {res[1]}")
    files, index = res[1], res[2]
    if include:
        files = [f for f in files if any(f["path"].endswith(x) for x in include)]
    return files, index


def _header(buf: torch.Tensor) -> bytes:
    (hlen,) = struct.unpack("<Q", buf[:8].cpu().numpy().tobytes())
    if 8 + hlen > buf.numel():
        raise ValueError("safetensors header reaches past the file")
    return buf[:8 + hlen].cpu().numpy().tobytes()


def _plans(entries, sh):
    """entries: [(path, size, slot offset, header)] of one owner's round -> [(path, plan, slot offset,
    offset of the file's part in the owner's part of the round arena)], bytes of that part.  Sender
    and receiver both lay a part out with this."""
    out, pos = [], 0
    for path, size, slot, head in entries:
        start, meta = zdev.parse_safetensors_header(head)
        plan = zshard.plan_file(start, meta, sh, size)
        out.append((path, plan, slot, pos))
        pos += _align(plan.arena_bytes)
    return out, pos


def _shifted(plan, slot: int, pos: int) -> np.ndarray:
    t = plan.table.copy()
    t["src_off"] += np.uint64(slot)
    t["dst_off"] += np.uint64(pos)
    return t


def _empty(n: int, dev: torch.device) -> torch.Tensor:
    return ops.padded_empty(n, dev) if dev.type == "cuda" else torch.empty(n, dtype=torch.uint8)


def swarm_pull_sharded(repo: str, revision: str = "main", group=None, device=None, shard=None, *,
                       scratch_bytes: int | None = None, exchange: str = "auto", cross_check: bool | None = None,
                       stats: dict | None = None, p2p: bool = True, peers=None, tracker=None, dht: bool = True,
                       dht_bootstrap=None, repo_type: str = "model", staging_bytes: int = 1 << 30, threads: int = 16,
                       include=None) -> dict[str, torch.Tensor]:
    """Collective over `group`: returns this rank's slices {tensor_name: tensor} on its device (see
    the module docstring).  `shard`: a Shard or (rank, world) whose rank and world equal the
    group's; a mismatch on any rank is agreed on before any fetch and every rank raises ValueError.
    `exchange`: "auto" ("mapped" on GPUs at world <= 16 when every rank mapped every peer, else
    "send"; ZEST_SHARD_EXCHANGE overrides it), "mapped" or "send".  `cross_check` (default
    ZEST_SHARD_CROSSCHECK=1): run both paths every round, compare every kept byte on the device,
    raise on a difference, count cross_checked_bytes.  `stats["shard"]` receives file_bytes,
    kept_bytes, skipped_files, groups, scratch_bytes, gather_s, exchange, rounds, owned_files,
    fetched_bytes (file bytes this rank pulled from the network), received_bytes (kept bytes that
    came from other ranks' scratches) and p2p_ratio (received_bytes / kept_bytes)."""
    if exchange not in EXCHANGES:
        raise ValueError(f"exchange={exchange!r}: a collective sharded pull takes one of {', '.join(EXCHANGES)}")
    if shard is None:
        raise ValueError("swarm_pull_sharded needs shard=")
    if not dist.is_initialized():
        raise ValueError("swarm_pull_sharded needs an initialised process group (zest_amd.parallel.init_from_env)")
    sh = zshard.as_shard(shard)
    if cross_check is None:
        cross_check = os.environ.get("ZEST_SHARD_CROSSCHECK", "0") == "1"
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device()) \
            if str(dist.get_backend(group)).lower() == "nccl" else torch.device("cpu")
    dev = torch.device(device)
    if dev.type not in ("cuda", "cpu"):
        raise ValueError("swarm_pull_sharded needs a GPU or the CPU")
    cuda = dev.type == "cuda"
    ctl = _Ctl(group, dev)
    rank, world = ctl.rank, ctl.world
    said = ctl.gather((sh.rank, sh.world))
    wrong = [r for r, v in enumerate(said) if tuple(v) != (r, world)]
    if wrong:
        raise ValueError(f"shard= does not match the process group on rank(s) {wrong}: rank {wrong[0]} of {world} "
                         f"passed Shard(rank={said[wrong[0]][0]}, world={said[wrong[0]][1]})")
    if exchange == "auto":
        exchange = os.environ.get("ZEST_SHARD_EXCHANGE", "auto")
        if exchange not in EXCHANGES:
            raise ValueError(f"ZEST_SHARD_EXCHANGE={exchange!r}: one of {', '.join(EXCHANGES)}")
    if (exchange == "mapped" or cross_check) and not cuda:
        raise ValueError("exchange='mapped' (and cross_check) read peers' device memory: they need GPUs")

    net = (p2p, list(peers or []), tracker, dht, list(dht_bootstrap or []))
    files, index = _listing(ctl, repo, revision, repo_type, net, include)
    st_files = [f for f in files if f["path"].endswith(".safetensors")]
    skipped: set = set()
    if index is not None and st_files:  # skip a file only when no rank keeps anything of it
        names = [f["path"] for f in st_files]
        skipped = set(names)
        for r in range(world):
            skipped &= zshard.files_to_skip(index, names, zshard.Shard(r, world, sh.plan))
        st_files = [f for f in st_files if f["path"] not in skipped]
    xet = [f for f in st_files if f["xet_hash"]]
    plain = [f for f in st_files if not f["xet_hash"]]
    owner = assign_owners([f["size"] for f in xet], world)
    mine = [f for f, o in zip(xet, owner) if o == rank]

    out: dict[str, torch.Tensor] = {}
    info = {"file_bytes": 0, "kept_bytes": 0, "skipped_files": sorted(skipped), "groups": 0, "scratch_bytes": 0,
            "gather_s": 0.0, "exchange": exchange, "rounds": 0, "owned_files": [f["path"] for f in mine],
            "fetched_bytes": 0, "received_bytes": 0, "p2p_ratio": 0.0, "round_gather_s": []}
    if cross_check:
        info["cross_checked_bytes"] = 0
    groups, scratch_n = [], 0
    if mine:
        biggest = max(direct._slot(f["size"]) for f in mine)
        want = max(max(f["size"] for f in mine), direct.DEFAULT_SCRATCH) if scratch_bytes is None \
            else int(scratch_bytes)
        scratch_n = min(max(want, biggest), sum(direct._slot(f["size"]) for f in mine))
        groups = direct._groups(mine, scratch_n)
    info["groups"], info["scratch_bytes"] = len(groups), scratch_n
    rounds = max(ctl.gather(len(groups)))
    info["rounds"] = rounds

    mapped = None
    scratch = None
    if xet:
        want_map = cuda and world <= ops.MAX_SLICE_SRCS and (exchange in ("auto", "mapped") or cross_check)
        if exchange == "mapped" and world > ops.MAX_SLICE_SRCS:
            raise ValueError(f"exchange='mapped' serves at most {ops.MAX_SLICE_SRCS} ranks")
        if cuda:
            with torch.cuda.device(dev):
                scratch = ops.vmm_empty(max(scratch_n, ops.PAD), dev) if want_map else \
                    ops.padded_empty(max(scratch_n, ops.PAD), dev)
                torch.cuda.synchronize(dev)  # the allocation is visible to the pull's private stream
        else:
            scratch = torch.empty(max(scratch_n, 1), dtype=torch.uint8)
        if want_map:
            if world == 1:
                mapped = [None]
            else:
                with torch.cuda.device(dev):
                    pa = zx.map_peer_arenas(scratch, rank, world, group=group)
                mapped = pa.peers if pa is not None else None
            if mapped is None and (exchange == "mapped" or cross_check):
                raise ShardPullError("exchange='mapped': the ranks could not map each other's scratch "
                                     "(exchange.map_peer_arenas); use exchange='send'")
        if exchange == "auto":
            exchange = "mapped" if mapped is not None else "send"
        info["exchange"] = exchange
    elif exchange == "auto":
        info["exchange"] = exchange = "send"

    fetcher = None  # made inside the first round's try: a rank that cannot build it fails like a failed pull
    timed = []  # cuda: (start, end) events around each round's gathers, read once at the end

    def add_views(path: str, plan, arena: torch.Tensor, theirs: bool) -> None:
        for k, v in plan.views(arena).items():
            if k in out:
                raise ValueError(f"duplicate tensor {k} in {path}")
            out[k] = v
        kept = sum(t.nbytes for t in plan.tensors)
        info["kept_bytes"] += kept
        if theirs:
            info["received_bytes"] += kept

    for j in range(rounds):
        g = groups[j] if j < len(groups) else []
        entries, err = [], None
        try:  # the owner pulls its group whole: every file keeps its Merkle check and CDN repair pass
            if g:
                if fetcher is None:
                    fetcher = ops.hip().DeviceXetPull(repo, revision, repo_type, *net, dev.index or 0, staging_bytes,
                                                      threads) if cuda else \
                        _core.HostXetFetcher(repo, revision, repo_type, *net, threads)
                jobs = [(f["xet_hash"], scratch.data_ptr() + o, f["size"]) for f, o in g]
                if cuda:
                    with torch.cuda.device(dev):
                        fetcher.pull_files(jobs)
                        torch.cuda.synchronize(dev)
                else:
                    fetcher.fetch_files(jobs)
                info["fetched_bytes"] += sum(f["size"] for f, _ in g)
                entries = [(f["path"], f["size"], o, _header(scratch[o:o + f["size"]])) for f, o in g]
        except Exception as e:  # noqa: BLE001  (agreed on below; no rank is left in a later collective)
            err = e
        bad = ctl.failed(err is not None)
        if bad:
            if err is not None:
                raise err
            raise ShardPullError(f"rank {rank}: rank(s) {bad} could not pull or verify their files of round {j}")
        shared = ctl.gather(entries)  # the round's headers, by owner
        info["file_bytes"] += sum(e[1] for ent in shared for e in ent)
        with torch.cuda.device(dev) if cuda else contextlib.nullcontext():
            if cuda:
                ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                ev0.record()
            t0 = time.perf_counter()
            if exchange == "mapped":
                got = _round_mapped(shared, sh, rank, scratch, mapped, dev)
            else:
                got = _round_send(shared, sh, ctl, scratch, dev)
            if cuda:
                ev1.record()
                timed.append((ev0, ev1))
            if cross_check:  # the other path into a second arena, compared byte for byte on the device
                other = _round_send(shared, sh, ctl, scratch, dev) if exchange == "mapped" else \
                    _round_mapped(shared, sh, rank, scratch, mapped, dev)
                try:
                    info["cross_checked_bytes"] += _compare(got, other, rank, j)
                except ShardPullError as e:
                    err = e
                del other
            if cuda:
                torch.cuda.current_stream(dev).synchronize()
            else:
                info["round_gather_s"].append(time.perf_counter() - t0)
        for o, parts in enumerate(got):
            for path, plan, arena in parts:
                add_views(path, plan, arena, o != rank)
        if mapped is not None and world > 1:
            # Every reader's gather has finished (synchronised above) before any owner's next pull
            # overwrites the scratch it read; a failed cross-check is agreed on in the same all-reduce.
            bad = ctl.failed(err is not None)
            if err is not None:
                raise err
            if bad:
                raise ShardPullError(f"rank {rank}: the cross-check of round {j} failed on rank(s) {bad}")
        elif err is not None:
            raise err
    del scratch
    if plain:  # non-Xet safetensors: every rank loads and gathers them itself
        direct._pull_plain_sharded(repo, revision, net, repo_type, plain, dev, sh, out, info)
    if timed:
        torch.cuda.synchronize(dev)
        info["round_gather_s"] = [a.elapsed_time(b) / 1e3 for a, b in timed]
    info["gather_s"] += sum(info["round_gather_s"])
    info["p2p_ratio"] = info["received_bytes"] / info["kept_bytes"] if info["kept_bytes"] else 0.0
    if stats is not None:
        stats["shard"] = info
    return out


def _round_mapped(shared, sh, rank: int, scratch, mapped, dev):
    """One K11 launch: this rank's slices of every file of the round, out of the owners' scratches
    (its own, and the peers' mappings) into one new compact arena.  Returns, per owner, [(path,
    plan, the file's part of the arena)]."""
    srcs, tables, laid, pos = [], [], [], 0
    for o, entries in enumerate(shared):
        plans, n = _plans(entries, sh)
        srcs.append(scratch if o == rank else mapped[o])
        tables.append(np.concatenate([_shifted(p, slot, pos + off) for _, p, slot, off in plans])
                      if plans else np.zeros(0, dtype=ops.SLICE_DTYPE))
        laid.append([(path, p, pos + off) for path, p, _, off in plans])
        pos += n
    arena = _empty(pos, dev)
    ops.slice_gather_peers(srcs, tables, arena)
    return [[(path, p, arena[off:off + p.arena_bytes]) for path, p, off in parts] for parts in laid]


def _round_send(shared, sh, ctl: _Ctl, scratch, dev):
    """The owner gathers every destination's slices of its files into a send buffer (one K10 launch,
    outputs laid out destination by destination) and the parts are moved; this rank's own part is
    gathered straight into its arena.  Same return value as _round_mapped."""
    rank, world = ctl.rank, ctl.world
    recv_plans = [_plans(entries, sh) for entries in shared]  # what this rank receives, by owner
    sizes_in = [0 if o == rank else n for o, (_, n) in enumerate(recv_plans)]
    sizes_out, tabs, pos = [0] * world, [], 0
    for r in range(world):  # what this rank sends: its own files, planned for every other rank
        if r == rank or not shared[rank]:
            continue
        plans, n = _plans(shared[rank], zshard.Shard(r, world, sh.plan))
        tabs += [_shifted(p, slot, pos + off) for _, p, slot, off in plans]
        sizes_out[r] = n
        pos += n
    send = _empty(pos, dev)
    if tabs:
        ops.slice_gather(scratch, np.concatenate(tabs), send)
    own_plans, own_n = recv_plans[rank]
    own = _empty(own_n, dev)
    if own_plans:
        ops.slice_gather(scratch, np.concatenate([_shifted(p, slot, off) for _, p, slot, off in own_plans]), own)
    recv = _empty(sum(sizes_in), dev)
    _move(ctl, send, sizes_out, recv, sizes_in, dev)
    out, pos = [], 0
    for o, (plans, n) in enumerate(recv_plans):
        base, start = (own, 0) if o == rank else (recv, pos)
        out.append([(path, p, base[start + off:start + off + p.arena_bytes]) for path, p, _, off in plans])
        if o != rank:
            pos += n
    return out


def _move(ctl: _Ctl, send, sizes_out, recv, sizes_in, dev) -> None:
    """Part r of `send` to rank r, part o of `recv` from rank o.  RCCL: one all_to_all_single on the
    device buffers.  gloo has no all-to-all and carries host memory only: batch_isend_irecv, with
    device buffers staged through the host."""
    if ctl.world == 1:
        return
    if ctl.backend != "gloo":
        dist.all_to_all_single(recv, send, sizes_in, sizes_out, group=ctl.group)
        return
    host = dev.type != "cpu"
    s = send.cpu() if host else send
    r = torch.empty(recv.numel(), dtype=torch.uint8) if host else recv
    ops_, a, b = [], 0, 0
    for p in range(ctl.world):
        if sizes_out[p]:
            ops_.append(dist.P2POp(dist.isend, s[a:a + sizes_out[p]], ctl.global_ranks[p], group=ctl.group))
        a += sizes_out[p]
        if sizes_in[p]:
            ops_.append(dist.P2POp(dist.irecv, r[b:b + sizes_in[p]], ctl.global_ranks[p], group=ctl.group))
        b += sizes_in[p]
    for w in dist.batch_isend_irecv(ops_) if ops_ else []:
        w.wait()
    if host:
        recv.copy_(r)


def _compare(a, b, rank: int, round_no: int) -> int:
    """Every kept tensor byte of the two paths' results, compared on the device; returns the bytes."""
    n = 0
    for pa, pb in zip(a, b):
        for (path, plan, xa), (_, _, xb) in zip(pa, pb):
            for t in plan.tensors:
                if t.nbytes and not torch.equal(xa[t.dst_off:t.dst_off + t.nbytes], xb[t.dst_off:t.dst_off + t.nbytes]):
                    raise ShardPullError(f"rank {rank}: cross-check of round {round_no}: {t.name} of {path} differs "
                                         f"between the mapped and the send exchange")
                n += t.nbytes
    return n
