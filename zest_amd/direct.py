"""Device-direct pull: Xet files go from the network (peers / CDN / local xorb cache) to HBM with
GPU-side decode and verification (`_hip.DeviceXetPull`); the host only moves compressed bytes.

    tensors = pull_to_device("meta-llama/Llama-3.1-8B", device="cuda:0")
    tensors = pull_to_device("meta-llama/Llama-3.1-8B", device="cpu")   # in memory, no disk

device="cpu": the same fetch through the host waterfall straight into CPU tensors
(`_core.HostXetFetcher`: CPU decode + BLAKE3/Merkle verification, no snapshot written).

Non-Xet files of the repo (config, tokenizer, small safetensors) are fetched by the native host
pull (`include=` filter) and loaded like the disk path.  With `save_snapshot=True` the verified
device bytes are also written to the HF cache snapshot so later `from_pretrained` calls hit disk.

    tensors = pull_to_device("meta-llama/Llama-3.1-8B", device="cuda:0", seed=True)

`seed=True` (or a port number): once the files have verified, their xorbs are served to BEP XET
peers straight from the HBM the returned tensors live in (`zest_amd.seed.ResidentSeedServer`): no
serialized second copy, no disk.  The server is kept in `zest_amd.seed.active()` until
`zest_amd.seed.stop_all()`.  Treat the tensors as read-only while seeding.

    tensors = pull_to_device("meta-llama/Llama-3.1-405B", device="cuda:3", shard=(3, 8))

`shard=` (a `zest_amd.shard.Shard`, or (rank, world) for the built-in "llama-tp" plan): only this
rank's tensor slices stay in device memory.  Files are still pulled and verified whole (a Xet file
hash covers every chunk of the file) through one reused scratch of `scratch_bytes`, then
`ops.slice_gather` copies the kept slices into a compact arena per file; files in which the rank
keeps nothing (per `model.safetensors.index.json`) are not fetched.  It bounds device memory, not
network bytes (the collective `pull(device="all", shard=...)`, zest_amd.parallel.shard_pull,
does).  `stats["shard"]` receives file_bytes, kept_bytes, skipped_files, groups, scratch_bytes and
gather_s.

    pull_to_device("meta-llama/Llama-3.1-70B", "v2", device="cuda:0", into=model)

`into=` (a {checkpoint tensor name: destination tensor} dict or a torch.nn.Module): the same flow,
but after a group of files verifies `ops.slice_scatter` copies the wanted tensors to the addresses
of tensors the caller already owns, so nothing but the scratch is allocated (zest_amd.into).
`cast=True` with it: tensors stored in another float dtype than their destination's (F32, F16, BF16)
are converted on the way by `ops.slice_scatter_cast`.  `base=` with it (what an earlier `into=` pull
returned, or any other base): the model is updated in place, only the changed chunks are fetched and
written, and the rest is verified where it lies.
"""
from __future__ import annotations

import os
import struct

import torch

from . import _core, ops
from . import device as zdev
from . import shard as zshard


def pull_to_device(repo: str, revision: str = "main", device="cuda:0", *, p2p: bool = True, peers=None,
                   tracker=None, dht: bool = True, dht_bootstrap=None, repo_type: str = "model",
                   save_snapshot: bool = False, staging_bytes: int = 1 << 30, threads: int = 16, include=None, seed=False,
                   shard=None, scratch_bytes: int | None = None, stats: dict | None = None, base=None, into=None,
                   strict: bool = True, cast: bool = False):
    if cast and into is None:
        raise ValueError("cast=True needs into=: the conversion is to the dtype of destinations the caller owns; a "
                         "plain pull returns the tensors in the checkpoint's dtype")
    if into is not None:
        if device is None:
            raise ValueError("into= needs a device: use device='cuda:N' (or 'cpu'), the device the destinations are on")
        if device == "all":
            raise ValueError("into= is not supported with device='all' (swarm pulls): run one process per GPU with "
                             "device='cuda:N' and that GPU's own destinations")
        if base is not None and cast:
            raise ValueError("base= is not supported with cast=True: converted destinations do not hold the stored "
                             "bytes, so nothing of them can be verified or kept; pull with cast=True without a base")
        if seed is not False and seed is not None:
            raise ValueError("into= is not supported with seed=: the file bytes do not stay resident as files; seed "
                             "from a plain device pull")
        if save_snapshot:
            raise ValueError("into= is not supported with save_snapshot=True: whole files never stay in memory; "
                             "write the snapshot with a plain pull(repo)")
    if base is not None:
        if device is None:
            raise ValueError("base= needs a device: a delta pull copies resident chunks inside device='cuda:N' (or "
                             "'cpu'); use the base's device")
        if device == "all":
            raise ValueError("base= is not supported with device='all' (swarm pulls): run the delta pull per GPU with "
                             "device='cuda:N' and that GPU's own base")
        if shard is not None:
            raise ValueError("base= is not supported with shard=: a sharded pull keeps no whole file resident to reuse "
                             "or to serve as the next base, and slices do not hold whole chunks; use an unsharded pull")
    if shard is not None:
        if device is None:
            raise ValueError("shard= needs a device: use device='cuda:N' (or 'cpu')")
        if device == "all":
            raise ValueError("pull_to_device is the single-process pull: with shard= run one process per GPU with "
                             "device='cuda:N', or the collective zest_amd.pull(device='all', shard=...) "
                             "(zest_amd.parallel.swarm_pull_sharded)")
        if seed is not False and seed is not None:
            raise ValueError("shard= is not supported with seed=: the file bytes do not stay resident; seed from "
                             "an unsharded pull")
        if save_snapshot:
            raise ValueError("shard= is not supported with save_snapshot=True: whole files never stay in memory; "
                             "write the snapshot with a plain pull(repo)")
    dev = torch.device(device)
    if dev.type not in ("cuda", "cpu"):
        raise ValueError("pull_to_device needs a GPU or the CPU")
    if into is not None:
        from .into import pull_into

        rs = None
        if base is not None:  # refusals first; a Landed is bound here, to its destinations as they are now
            from . import delta as zdelta

            rs = zdelta.as_resident_set(base, dev)
        return pull_into(repo, revision, dev, into, None if shard is None else zshard.as_shard(shard), scratch_bytes,
                         stats, strict, p2p=p2p, peers=peers, tracker=tracker, dht=dht, dht_bootstrap=dht_bootstrap,
                         repo_type=repo_type, staging_bytes=staging_bytes, threads=threads, include=include, cast=cast,
                         base=rs)
    if shard is not None:
        return _pull_sharded(repo, revision, dev, zshard.as_shard(shard), scratch_bytes, stats, p2p=p2p, peers=peers,
                             tracker=tracker, dht=dht, dht_bootstrap=dht_bootstrap, repo_type=repo_type,
                             staging_bytes=staging_bytes, threads=threads, include=include)
    seed_port = None
    if seed is not False and seed is not None:
        from .seed import seed_port as _seed_port

        seed_port = _seed_port(seed)
        if dev.type != "cuda":
            raise ValueError(f"seed= serves weights resident in GPU memory: unsupported with device={str(device)!r}")
    rs = None
    if base is not None:  # refusals first: nothing is listed or allocated for a base that cannot serve
        from . import delta as zdelta

        rs = zdelta.as_resident_set(base, dev)
    commit, files = _core.list_repo_files(repo, revision, repo_type)
    if include:  # file-name suffixes, as `zest pull --include` (csrc/core/pull.cpp)
        files = [f for f in files if any(f["path"].endswith(x) for x in include)]
    st_files = [f for f in files if f["path"].endswith(".safetensors")]
    xet = [f for f in st_files if f["xet_hash"]]
    plain = [f for f in st_files if not f["xet_hash"]]
    out = zdev.Weights()
    resident = []  # (buffer, chunk_lens, term_keys) per Xet file: what seeding and the next delta pull need
    if xet and dev.type == "cpu":
        hf = _core.HostXetFetcher(repo, revision, repo_type, p2p, list(peers or []), tracker, dht,
                                  list(dht_bootstrap or []), threads)
        if rs is not None:
            resident = zdelta.pull_files_delta(hf, xet, dev, rs, _delta_info(stats))
        else:
            bufs = [torch.empty(f["size"], dtype=torch.uint8) for f in xet]
            res = hf.fetch_files([(f["xet_hash"], b.data_ptr(), f["size"]) for f, b in zip(xet, bufs)])
            resident = [(b, r["chunk_lens"], hf.term_keys(f["xet_hash"])) for f, b, r in zip(xet, bufs, res)]
    elif xet:
        dp = ops.hip().DeviceXetPull(repo, revision, repo_type, p2p, list(peers or []), tracker, dht,
                                     list(dht_bootstrap or []), dev.index or 0, staging_bytes, threads)
        if rs is not None:
            with torch.cuda.device(dev):
                resident = zdelta.pull_files_delta(dp, xet, dev, rs, _delta_info(stats))
        else:
            bufs = [ops.padded_empty(f["size"], dev)[:f["size"]] for f in xet]
            torch.cuda.synchronize(dev)  # allocations visible to the pull's private stream
            # one pipeline for all files: staging batches cross file boundaries
            res = dp.pull_files([(f["xet_hash"], b.data_ptr(), f["size"]) for f, b in zip(xet, bufs)])
            # the reconstructions are cached by the pull: listing their terms costs no request
            resident = [(b, r["chunk_lens"], dp.term_keys(f["xet_hash"])) for f, b, r in zip(xet, bufs, res)]
        if seed_port is not None:  # the files verified: serve their xorbs from where they now live
            from . import seed as zseed

            zseed._active.append(zseed.ResidentSeedServer(resident, dev, seed_port))
    for f, (buf, _, _) in zip(xet, resident):
        _add_views(out, buf, f["path"])
        if save_snapshot:
            _save(repo, commit or revision, f["path"], buf)
    out._set_files(resident, dev, meta=[(f["path"], f["xet_hash"]) for f in xet])
    if plain or save_snapshot:
        inc = [f["path"] for f in plain] + ([f["path"] for f in files if not f["path"].endswith(".safetensors")]
                                           if save_snapshot else [])
        if inc:
            r = _core.pull(repo, revision, p2p, list(peers or []), tracker, dht, list(dht_bootstrap or []), inc,
                           True, 0, repo_type)
            for f in plain:
                buf = zdev.load_file(os.path.join(r["snapshot_dir"], f["path"]), dev)
                _add_views(out, buf, f["path"])
    return out


def _delta_info(stats: dict | None) -> dict:
    """The dict that receives a delta pull's counters: stats["delta"] when the caller passed stats."""
    info: dict = {}
    if stats is not None:
        stats["delta"] = info
    return info


DEFAULT_SCRATCH = 16 << 30  # a default to revisit with measurements, not a tuned value


def _slot(size: int) -> int:
    """Scratch bytes of one file: its size rounded up to ops.PAD plus one more PAD (the decoders
    write wide, and a staging batch may cross file boundaries)."""
    return -(-size // ops.PAD) * ops.PAD + ops.PAD


def _groups(files, scratch: int):
    """Files in listing order, cut into groups whose slots fit `scratch`: [(file, slot offset), ...]."""
    out, cur, pos = [], [], 0
    for f in files:
        s = _slot(f["size"])
        if cur and pos + s > scratch:
            out.append(cur)
            cur, pos = [], 0
        cur.append((f, pos))
        pos += s
    if cur:
        out.append(cur)
    return out


def _pull_sharded(repo, revision, dev, sh, scratch_bytes, stats, *, p2p, peers, tracker, dht, dht_bootstrap, repo_type,
                  staging_bytes, threads, include):
    """pull_to_device(shard=...): whole files are pulled and verified (a Xet file hash is a Merkle
    root over every chunk of the file) into one reused scratch, group by group; after a group
    verifies, only the rank's slices are copied out (ops.slice_gather) into one compact arena per
    file, and the scratch is reused.  Bounds device memory, not network bytes."""
    import time

    net = (p2p, list(peers or []), tracker, dht, list(dht_bootstrap or []))
    commit, files = _core.list_repo_files(repo, revision, repo_type)
    has_index = any(f["path"] == zshard.INDEX_NAME for f in files)
    if include:
        files = [f for f in files if any(f["path"].endswith(x) for x in include)]
    st_files = [f for f in files if f["path"].endswith(".safetensors")]
    skipped: set = set()
    if has_index and st_files:  # which file holds which tensor, without fetching any of them
        r = _core.pull(repo, revision, *net, [zshard.INDEX_NAME], True, 0, repo_type)
        with open(os.path.join(r["snapshot_dir"], zshard.INDEX_NAME), "rb") as fh:
            skipped = zshard.files_to_skip(fh.read(), [f["path"] for f in st_files], sh)
        st_files = [f for f in st_files if f["path"] not in skipped]
    xet = [f for f in st_files if f["xet_hash"]]
    plain = [f for f in st_files if not f["xet_hash"]]
    cuda = dev.type == "cuda"
    out: dict[str, torch.Tensor] = {}
    info = {"file_bytes": 0, "kept_bytes": 0, "skipped_files": sorted(skipped), "groups": 0, "scratch_bytes": 0,
            "gather_s": 0.0}
    timed = []  # cuda: (start, end) events around each group's gathers, read once at the end

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
                    # one pipeline per group: staging batches cross file boundaries, every file keeps its
                    # Merkle check and CDN repair pass
                    dp.pull_files([(f["xet_hash"], scratch.data_ptr() + o, f["size"]) for f, o in g])
                    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    ev0.record()
                    for f, o in g:
                        _gather_file(scratch[o:o + f["size"]], f["path"], sh, dev, out, info)
                    ev1.record()
                    timed.append((ev0, ev1))
                    # The next group overwrites the scratch these gathers read.  Only the pipeline's
                    # compute stream writes caller memory (its H2D copies land in its own staging), so
                    # queueing that stream behind the gathers' event is enough: no host sync.
                    dp.order_after(ev1.cuda_event)
                del scratch  # back to torch's allocator, which orders its reuse behind the gathers' stream
        else:
            hf = _core.HostXetFetcher(repo, revision, repo_type, *net, threads)
            scratch = torch.empty(scratch_n, dtype=torch.uint8)
            for g in groups:
                hf.fetch_files([(f["xet_hash"], scratch.data_ptr() + o, f["size"]) for f, o in g])
                t0 = time.perf_counter()
                for f, o in g:
                    _gather_file(scratch[o:o + f["size"]], f["path"], sh, dev, out, info)
                info["gather_s"] += time.perf_counter() - t0
    if plain:
        _pull_plain_sharded(repo, revision, net, repo_type, plain, dev, sh, out, info)
    if timed:
        torch.cuda.synchronize(dev)
        info["gather_s"] += sum(a.elapsed_time(b) for a, b in timed) / 1e3
    if stats is not None:
        stats["shard"] = info
    return out


def _gather_file(buf: torch.Tensor, path: str, sh, dev, out: dict, info: dict) -> None:
    """Plan one verified file in `buf` for `sh`, gather the kept slices into a new arena and add the
    views to `out`; counts file_bytes and kept_bytes in `info`."""
    (hlen,) = struct.unpack("<Q", buf[:8].cpu().numpy().tobytes())
    start, meta = zdev.parse_safetensors_header(buf[:8 + hlen].cpu().numpy().tobytes())
    plan = zshard.plan_file(start, meta, sh, buf.numel())
    arena = ops.padded_empty(plan.arena_bytes, dev) if dev.type == "cuda" else \
        torch.empty(plan.arena_bytes, dtype=torch.uint8)
    ops.slice_gather(buf, plan.table, arena)
    for k, v in plan.views(arena).items():
        if k in out:
            raise ValueError(f"duplicate tensor {k} in {path}")
        out[k] = v
    info["file_bytes"] += buf.numel()
    info["kept_bytes"] += sum(t.nbytes for t in plan.tensors)


def _pull_plain_sharded(repo, revision, net, repo_type, plain, dev, sh, out: dict, info: dict) -> None:
    """Non-Xet safetensors of a sharded pull (single-process and collective alike): the host route,
    then the same plan and gather, file by file.  Adds the gather time to info["gather_s"]."""
    import time

    r = _core.pull(repo, revision, *net, [f["path"] for f in plain], True, 0, repo_type)
    for f in plain:
        buf = zdev.load_file(os.path.join(r["snapshot_dir"], f["path"]), dev)
        t0 = time.perf_counter()
        if dev.type == "cuda":
            with torch.cuda.device(dev):
                _gather_file(buf, f["path"], sh, dev, out, info)
                torch.cuda.current_stream(dev).synchronize()  # buf is freed before the next file loads
        else:
            _gather_file(buf, f["path"], sh, dev, out, info)
        info["gather_s"] += time.perf_counter() - t0
        del buf


def _add_views(out: dict, buf: torch.Tensor, path: str) -> None:
    (hlen,) = struct.unpack("<Q", buf[:8].cpu().numpy().tobytes())
    start, meta = zdev.parse_safetensors_header(buf[:8 + hlen].cpu().numpy().tobytes())
    for k, v in zdev.tensor_views(buf, start, meta).items():
        if k in out:
            raise ValueError(f"duplicate tensor {k} in {path}")
        out[k] = v


def _save(repo: str, commit: str, path: str, buf: torch.Tensor) -> None:
    import json

    cfg = json.loads(_core.config_json())
    snap = os.path.join(cfg["hf_cache_dir"], _core.repo_folder_name(repo), "snapshots", commit)
    dst = os.path.join(snap, path)
    os.makedirs(os.path.dirname(dst), exist_ok=True)
    tmp = dst + ".incomplete"
    buf.cpu().numpy().tofile(tmp)
    os.replace(tmp, dst)
