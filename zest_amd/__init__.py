"""zest_amd — MI355X-native P2P model distribution (zest capabilities, rebuilt for AMD CDNA4).

Usage (same API as the reference's `zest` package, python/zest/__init__.py:1-73):

    import zest_amd as zest          # or: import zest  (compat shim)
    zest.enable()                    # background seeder + huggingface_hub patch
    path = zest.pull("meta-llama/Llama-3.1-8B")
    weights = zest.pull("meta-llama/Llama-3.1-8B", device="cuda:0")   # HBM tensors, GPU-verified
    model = zest.from_pretrained("meta-llama/Llama-3.1-8B")            # transformers model on those tensors
    print(zest.status()); zest.stop()

Layers (see docs/ARCHITECTURE.md):
  zest_amd._core    C++17 host core: BLAKE3/Xet hashing, LZ4/BG4, CDC, xorbs, BT/DHT/HTTP stack
  zest_amd._hip     HIP/CDNA4 kernels for gfx950: xorb ingest (decode+verify), BLAKE3, Merkle, CDC
  zest_amd.ops      torch-facing wrappers of the HIP kernels
  zest_amd.parallel RCCL (torch.distributed "nccl") intra-node swarm: GPUs as BitTorrent peers
  zest_amd.models   synthetic model specs (gpt2, Llama-3.1-8B/70B, Qwen2-7B, Mixtral-8x7B)
  zest_amd.utils    tracing, fault-injection spec, formatting helpers
"""
from __future__ import annotations

import os

__version__ = "0.4.2"

_server = None
_client = None


def _init():
    global _server, _client
    if _server is None:
        from .client import ZestClient
        from .server import ZestServer

        _server = ZestServer()
        _client = ZestClient()


def enable() -> None:
    """Start the background zest server (seeding) and route huggingface_hub downloads through zest."""
    _init()
    _server.ensure_running()
    from .hf_backend import patch_hf_hub

    patch_hf_hub(_client)


def disable() -> None:
    """Restore the original huggingface_hub functions."""
    from .hf_backend import unpatch_hf_hub

    unpatch_hf_hub()


def pull(repo: str, revision: str = "main", *, device=None, as_tensors: bool = False, verify: bool = True,
         p2p: bool = True, peers=None, tracker=None, dht: bool = True, dht_bootstrap=None, include=None,
         group=None, repo_type: str = "model", verbose: bool = False, direct: bool | None = None,
         save_snapshot: bool = False, threads: int = 16, staging_bytes: int = 1 << 30, stats: dict | None = None,
         exchange: str = "auto", round_bytes: int | None = None, seed=False, shard=None,
         scratch_bytes: int | None = None, base=None, into=None, strict: bool = True, cast: bool = False):
    """Download `repo@revision` via zest.

    * default: returns the HF-cache snapshot directory (reference behaviour).
    * device="cuda:N" (or as_tensors=True): also loads every *.safetensors file into that GPU's HBM,
      verifies each against its Xet file hash on the GPU, and returns {tensor_name: tensor}.
    * device="all": collective over `group` (default WORLD) — every rank gets all tensors on its
      own GPU (CPU process groups: host memory).  The model's reconstruction terms are split into
      byte-balanced per-rank shares; each rank fetches its share device-direct, round by round,
      and the rounds are replicated over xGMI with the exchange strategy measured fastest at setup
      (`exchange`, default "auto"), every received chunk re-hashed on the receiver, every file
      Merkle-checked on every rank; no snapshot is written (zest_amd.parallel.swarm_pull).
      `stats` (a dict) receives the exchange mode used, bytes fetched / received, per-phase
      seconds, re-shards and recovered ranks.
    * device="cuda:N" / "cpu" pulls are device-direct by default (`direct=None` -> True, like
      from_pretrained): Xet files bypass the disk -- fetched compressed through the
      cache/peer/CDN waterfall and decoded + hash-verified on the GPU into HBM (zest_amd.direct);
      `threads` fetch workers fill pinned staging buffers of `staging_bytes` each.  With
      device="cpu" the same pull lands in CPU tensors (host decode + verification, no disk).  No
      snapshot is written unless `save_snapshot=True`; `include` (file-name suffixes) filters the
      safetensors files.  direct=False: the reference's path -- the CLI writes the HF-cache
      snapshot, which is then loaded and (verify=True) hash-checked on the device.
    * seed=True (or a port number), single-GPU direct pulls only: after the files verify, their xorbs
      are seeded to BEP XET peers straight from the HBM the returned tensors occupy -- no serialized
      copy, no disk (zest_amd.seed.ResidentSeedServer; `zest_amd.seed.active()` lists the servers,
      `zest_amd.seed.stop_all()` / `zest_amd.stop()` stop them).  Keep the tensors read-only meanwhile.
    * shard=Shard(rank, world, plan) or (rank, world), device="cuda:N" / "cpu" direct pulls: the
      returned tensors are this rank's slices (tensor-parallel parts, a pipeline stage, its experts:
      zest_amd.shard) and only they stay in device memory.  Every file is still pulled and verified
      whole, through a reused scratch of `scratch_bytes` (default: the larger of the largest file and
      16 GiB, never more than the files need), because a Xet file hash covers the whole file: this
      bounds device memory, not network bytes.  Files in which the rank keeps nothing (per
      model.safetensors.index.json) are not fetched.  `stats["shard"]` receives file_bytes, kept_bytes,
      skipped_files, groups, scratch_bytes and gather_s.
    * base=w0 (the Weights an earlier direct pull returned, its `.resident` set, what
      `zest_amd.publish` returned, or a list of those),
      device="cuda:N" / "cpu" direct pulls: a delta pull.  Reconstruction terms of the new revision
      whose chunks are all resident in the base's memory on the same device are copied from there and
      re-hashed on the way (ops.reuse_chunks, kernel K12) instead of fetched; the rest takes the usual
      waterfall.  Every file is verified from the hashes of the bytes in its new buffer, so nothing
      about the base is trusted: a file that misses (base tensors modified in place) has its reused
      terms fetched from the network and is checked again.  The base is not updated in place: old and
      new weights coexist until the caller drops the old ones.  seed=True serves the new revision from
      HBM as usual.  `stats["delta"]` receives reused_terms, fetched_terms, reused_bytes, fetched_bytes,
      reused_files, refetched_terms, reuse_s, fetch_s and verify_s.  Refused with device="all", shard=,
      direct=False, no device, and a base on another device (zest_amd.delta).
    * shard= with device="all": the collective sharded pull over `group` (default WORLD; start one
      process per GPU and call zest_amd.parallel.init_from_env() first).  The shard's rank and world
      must be the group's.  Each file is fetched and verified whole by one owner rank and every rank
      takes only its own slices out of the owner's memory, so each file crosses the network once per
      group and only kept slices cross xGMI (zest_amd.parallel.shard_pull).  `exchange`: "auto",
      "mapped" (GPUs: one gather launch over the peer-mapped scratches) or "send" (gather on the
      owner, then all-to-all; any backend, CPU groups).  ZEST_SHARD_CROSSCHECK=1 runs both and compares
      every kept byte.  `stats["shard"]` also receives exchange, rounds, owned_files, fetched_bytes,
      received_bytes and p2p_ratio.  seed=, save_snapshot=True and direct=False stay refused.
    * into=target (a {checkpoint tensor name: destination tensor} dict or a torch.nn.Module, taken as
      its state_dict(keep_vars=True)), device="cuda:N" / "cpu" direct pulls: the tensors are written into
      memory the caller already owns, at fixed addresses, instead of into new buffers (zest_amd.into).
      Files are pulled and verified whole through the reused scratch of `scratch_bytes`, as with
      shard=, then ops.slice_scatter (kernel K15) copies each wanted tensor to its destination's address:
      peak device memory is the model plus one scratch, not two models.  No byte of a file reaches a
      destination before the whole file has passed its Xet hash; a file that fails, or whose tensors
      differ from their destinations in dtype or shape (ValueError naming the tensor), leaves its
      destinations untouched, while earlier files stay written.  Destinations are contiguous views
      on `device` that do not overlap; a fused parameter is passed as one view per checkpoint tensor;
      names that alias the same bytes (tied weights) are written once, under the first name.  With
      shard= each destination holds the rank's slice.  Checkpoint tensors that `into` does not name
      are not kept, and files that hold none of its names are not fetched.  strict=True (default):
      KeyError after the pull when no file provided a wanted name.  Returns {name: the destination
      passed in} for every tensor written, after the device has finished.  Autograd version counters
      are not bumped, and the caller must not run the model during the call.  `stats["into"]`
      receives file_bytes, written_bytes, tensors, skipped_files, missing, groups, scratch_bytes and
      scatter_s.  Refused with device="all", seed=, save_snapshot=True, direct=False and no device.
      The returned dict is a `zest_amd.into.Landed`: it also carries `.record`, plain data that says
      which chunks the destinations hold.
    * into=target with base= (the Landed of an earlier into= pull of the same destinations, or any
      other base): the model is updated in place.  Terms whose chunks all lie in the base are hashed
      where they lie (ops.hash_chunks_at), the others are fetched into a patch scratch; once the file's
      Merkle root equals its Xet hash, chunks already at their place are kept, other resident chunks are
      gathered and re-hashed (ops.reuse_chunks), and ops.slice_scatter writes only the fetched and the
      moved pieces.  Peak memory above the model is the changed bytes plus small tables.  A file that
      misses its hash (destinations modified since) wrote nothing and is pulled whole instead.  The
      returned Landed carries the new record, so calls chain.  `stats["into"]["delta"]` receives
      kept_terms, kept_bytes, moved_chunks, moved_bytes, fetched_terms, fetched_bytes, applied_bytes,
      seam_chunks, seam_bytes, patch_bytes, fallback_files, fallback_bytes, check_s, fetch_s, apply_s,
      bind_s (the part of check_s spent binding the record) and per-file counters under files.  Refused with shard= and cast=True.  A Landed is also a
      plain base: pull(repo, rev, device=..., base=landed) copies out of the model's tensors.
    * cast=True, with into= only: a wanted tensor stored in another float dtype than its destination's
      is converted on the way, F32, F16 and BF16 to each other (round to nearest even, overflow to
      infinity, subnormals kept, NaN stays NaN).  Files are verified in their stored dtype; per
      verified file the tensors whose dtype matches go through ops.slice_scatter as before and the
      others through one ops.slice_scatter_cast launch (kernel K16), so peak device memory stays the
      model plus one scratch, where pull() followed by a converting copy_ holds the whole checkpoint
      next to the model.  Any other dtype pair (integers, bool, F8, F64) is still refused with a
      ValueError naming the tensor, before anything of that file is written.  `stats["into"]` also
      receives cast_tensors and cast_bytes_in (stored bytes converted); written_bytes counts
      destination bytes.  cast=False (default) converts nothing.  Refused without into=.
    """
    if cast and into is None:
        raise ValueError("cast=True needs into=: the conversion is to the dtype of destinations the caller owns; a "
                         "plain pull returns the tensors in the checkpoint's dtype")
    if into is not None:
        if device is None:
            raise ValueError("into= needs a device: use device='cuda:N' (or 'cpu'), the device the destinations are "
                             "on; a snapshot pull has no tensors to place")
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
        if direct is False:
            raise ValueError("into= is not supported with direct=False (the snapshot path): use the default "
                             "device-direct pull, or load the snapshot and copy_ the tensors yourself")
    if base is not None:
        if device is None and not as_tensors:
            raise ValueError("base= needs a device pull: a snapshot pull lands on disk, where nothing is resident; use "
                             "device='cuda:N' (or 'cpu'), the device the base was pulled to")
        if device == "all":
            raise ValueError("base= is not supported with device='all' (swarm pulls): run the delta pull per GPU with "
                             "device='cuda:N' and that GPU's own base")
        if shard is not None:
            raise ValueError("base= is not supported with shard=: a sharded pull keeps no whole file resident to reuse "
                             "or to serve as the next base; use an unsharded pull")
        if direct is False:
            raise ValueError("base= is not supported with direct=False (the snapshot path): resident chunks are "
                             "copied into the buffers of a device-direct pull; leave direct at its default")
        if into is not None:  # every refusal of a base before any request; a Landed is bound here, once
            from .delta import as_resident_set

            base = as_resident_set(base, device)
    if shard is not None:
        if device is None:
            raise ValueError("shard= needs a device: use device='cuda:N' (or 'cpu'); a snapshot pull has no tensors "
                             "to slice")
        if device == "all":
            import torch.distributed as dist

            if group is None and not (dist.is_available() and dist.is_initialized()):
                raise ValueError("shard= with device='all' is a collective: start one process per GPU (torchrun), "
                                 "call zest_amd.parallel.init_from_env() in each, then pull(device='all', "
                                 "shard=(rank, world)); without a process group use device='cuda:N'")
            if seed is not False and seed is not None:
                raise ValueError("shard= is not supported with seed=: the file bytes do not stay resident; seed "
                                 "from an unsharded pull")
            if save_snapshot:
                raise ValueError("shard= is not supported with save_snapshot=True: whole files never stay in "
                                 "memory; write the snapshot with a plain pull(repo)")
            if exchange not in ("auto", "mapped", "send"):
                raise ValueError(f"exchange={exchange!r}: a collective sharded pull takes auto, mapped or send")
        if direct is False:
            raise ValueError("shard= is not supported with direct=False (the snapshot path): use the default "
                             "device-direct pull")
    if seed is not False and seed is not None:
        if device == "all":
            raise ValueError("seed= is not supported with device='all' (swarm pulls): use a single device='cuda:N'")
        if device is None and not as_tensors:
            raise ValueError("seed= needs a device pull (device='cuda:N'); snapshot pulls are seeded by the "
                             "background server")
        if direct is False:
            raise ValueError("seed= is not supported with direct=False (the snapshot path): it serves the "
                             "buffers of a device-direct pull")
    _init()
    kw = dict(p2p=p2p, peers=peers, tracker=tracker, dht=dht, dht_bootstrap=dht_bootstrap, include=include,
              verify=verify, repo_type=repo_type, verbose=verbose)
    if device is None and not as_tensors:
        return _client.pull(repo, revision, **kw)
    if device == "all" and shard is not None:
        from .parallel import swarm_pull_sharded

        return swarm_pull_sharded(repo, revision, group=group, shard=shard, scratch_bytes=scratch_bytes,
                                  exchange=exchange, stats=stats, p2p=p2p, peers=peers, tracker=tracker, dht=dht,
                                  dht_bootstrap=dht_bootstrap, repo_type=repo_type, staging_bytes=staging_bytes,
                                  threads=threads, include=include)
    if device == "all":
        from .parallel import swarm_pull

        return swarm_pull(repo, revision, group=group, p2p=p2p, peers=peers, tracker=tracker, dht=dht,
                          dht_bootstrap=dht_bootstrap, repo_type=repo_type, verify_received=verify,
                          staging_bytes=staging_bytes, threads=threads, stats=stats, exchange=exchange,
                          round_bytes=round_bytes)
    if direct is None:
        direct = True  # weights straight into device memory (the north star); direct=False: via disk
    if direct:
        from .direct import pull_to_device

        return pull_to_device(repo, revision, device or "cuda:0", p2p=p2p, peers=peers, tracker=tracker, dht=dht,
                              dht_bootstrap=dht_bootstrap, repo_type=repo_type, save_snapshot=save_snapshot,
                              threads=threads, staging_bytes=staging_bytes, include=include, seed=seed, shard=shard,
                              scratch_bytes=scratch_bytes,
                              stats=stats if shard is not None or base is not None or into is not None else None,
                              base=base, into=into, strict=strict, cast=cast)
    from .device import load_snapshot

    res = _client.pull_detailed(repo, revision, **kw)
    return load_snapshot(res.snapshot_dir, device or "cuda:0", res.xet_hashes() if verify else None)


def publish(files, **kw):
    """Publish files resident in GPU (or host) memory as a new, deduplicated Xet revision; see
    zest_amd.publish.publish.  (Once that module is imported `zest_amd.publish` names the module,
    which is callable with the same signature.)"""
    from .publish import publish as _publish

    return _publish(files, **kw)


def __getattr__(name: str):
    if name in ("ChunkIndex", "TensorFile"):  # lazy: importing the package does not import torch
        from . import publish as _pub

        return getattr(_pub, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def from_pretrained(repo: str, revision: str = "main", **kw):
    """transformers model built around weights pulled into `device` memory (zest_amd.hf_model)."""
    from .hf_model import from_pretrained as _fp

    return _fp(repo, revision, **kw)


def status() -> dict:
    """Status JSON of the background server (starting it if needed)."""
    _init()
    _server.ensure_running()
    return _client.status()


def stop() -> None:
    """Stop the background server and every resident seed server started by pull(..., seed=...)."""
    import sys

    zseed = sys.modules.get(__name__ + ".seed")
    if zseed is not None:
        zseed.stop_all()
    _init()
    _server.stop()


# Auto-enable when ZEST=1 is set (reference python/zest/__init__.py:68-73).
if os.environ.get("ZEST", "").strip().lower() in ("1", "true", "yes"):
    try:
        enable()
    except Exception:
        pass
