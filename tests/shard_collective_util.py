"""Shared by the collective sharded pull's tests (CPU and GPU): the several-source gather checked
against shard_model.gather_model, and a process group of rank processes that is started once and
runs scenarios (one collective pull each) in sequence.
"""
from __future__ import annotations

import os
import time

import numpy as np
import torch

import shard_model as M


# ------------------------------------------------------------------------------------------------
# ops.slice_gather_peers against the model
# ------------------------------------------------------------------------------------------------
def source_bytes(n: int, seed: int) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


def deal(specs, k: int, dst_step: int = 256):
    """`specs` ((run_bytes, n_runs, src_stride) per tensor) dealt over k sources in contiguous shares:
    [(src bytes, entries with dst_off absolute in one arena)], arena length.  Each source's outputs
    start at the next multiple of dst_step after the source before it."""
    parts, base, arena = [], 0, 0
    for s, idx in enumerate(np.array_split(np.arange(len(specs)), k)):
        entries, src_len, last = M.lay_out([specs[i] for i in idx], dst_step=dst_step)
        parts.append((source_bytes(src_len, 100 + s), [(so, rb, st, nr, do + base) for so, rb, st, nr, do in entries]))
        if last:
            arena = base + last
            base = -(-arena // dst_step) * dst_step
    return parts, arena


def check_gather_peers(ops, device, parts, arena_len: int, aligns=None, max_blocks: int = 0) -> None:
    """Run ops.slice_gather_peers on `device` and compare the whole destination, canaries included,
    with gather_model applied per source.  Source s sits aligns[s] (default s % 16) bytes past a
    16-byte boundary and ends with its allocation's logical range."""
    srcs, tables = [], []
    want = np.full(arena_len + 2 * M.GUARD, M.CANARY, dtype=np.uint8)
    for s, (src, entries) in enumerate(parts):
        align = (s % 16) if aligns is None else aligns[s]
        hold = torch.empty(align + len(src), dtype=torch.uint8, device=device)
        assert hold.data_ptr() % 16 == 0
        hold[align:].copy_(torch.from_numpy(src))
        srcs.append(hold[align:])
        tables.append(np.array(entries, dtype=ops.SLICE_DTYPE))
        for do, b in M.gather_model(src.tobytes(), entries).items():
            assert (want[M.GUARD + do:M.GUARD + do + len(b)] == M.CANARY).all(), "the case's outputs overlap"
            want[M.GUARD + do:M.GUARD + do + len(b)] = np.frombuffer(b, dtype=np.uint8)
    full = torch.full((arena_len + 2 * M.GUARD,), M.CANARY, dtype=torch.uint8, device=device)
    assert full.data_ptr() % 16 == 0
    ops.slice_gather_peers(srcs, tables, full[M.GUARD:M.GUARD + arena_len], max_blocks=max_blocks)
    got = full.cpu().numpy()
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{bad.size} bytes differ, first at arena offset {int(bad[0]) - M.GUARD}"


def check_refusals(ops, device) -> None:
    """Every refusal of ops.slice_gather_peers, each naming the source and the entry; nothing is written."""
    import pytest

    a = torch.zeros(100, dtype=torch.uint8, device=device)
    b = torch.zeros(40, dtype=torch.uint8, device=device)
    dst = torch.zeros(128, dtype=torch.uint8, device=device)
    tab = lambda *e: np.array(list(e), dtype=ops.SLICE_DTYPE)
    ops.slice_gather_peers([a, b], [tab((90, 10, 10, 1, 0)), tab((0, 4, 18, 3, 16), (40, 0, 0, 0, 32))], dst)  # legal
    with pytest.raises(ValueError, match="17 sources"):
        ops.slice_gather_peers([b] * 17, [tab()] * 17, dst)
    with pytest.raises(ValueError, match="source 1 entry 0.*past the source"):  # inside a, not inside b
        ops.slice_gather_peers([a, b], [tab((0, 4, 4, 1, 0)), tab((50, 10, 10, 1, 16))], dst)
    with pytest.raises(ValueError, match="source 1 entry 0.*overlaps"):
        ops.slice_gather_peers([a, b], [tab((0, 17, 17, 1, 0)), tab((0, 4, 4, 1, 16))], dst)
    with pytest.raises(ValueError, match="source 1 entry 0.*overlaps or precedes"):  # descends across sources
        ops.slice_gather_peers([a, b], [tab((0, 4, 4, 1, 64)), tab((0, 4, 4, 1, 32))], dst)
    with pytest.raises(ValueError, match="source 2 entry 1.*aligned"):
        ops.slice_gather_peers([a, b, a], [tab((0, 4, 4, 1, 0)), tab(), tab((0, 4, 4, 1, 16), (0, 4, 4, 1, 40))], dst)
    with pytest.raises(ValueError, match="2 sources but 1 tables"):
        ops.slice_gather_peers([a, b], [tab()], dst)
    with pytest.raises(ValueError, match="source 1 .*uint8"):
        ops.slice_gather_peers([a, b.view(torch.int16)], [tab(), tab()], dst)
    assert not dst.any()  # nothing was written by a refused call (nor by the legal one: the sources are zero)


# ------------------------------------------------------------------------------------------------
# plans by name (a callable plan cannot cross a process boundary by value)
# ------------------------------------------------------------------------------------------------
def stage_plan(name, shape, dtype):
    """Pipeline stages: layer i belongs to rank (i + 1) % world alone, everything else is replicated;
    nothing is split.  Sees rank and world through plan.shard."""
    s = stage_plan.shard
    if ".layers." not in name:
        return None
    return None if (int(name.split(".layers.")[1].split(".")[0]) + 1) % s.world == s.rank else "drop"


def stage_keeps(name: str, rank: int, world: int) -> bool:
    return ".layers." not in name or (int(name.split(".layers.")[1].split(".")[0]) + 1) % world == rank


DROPPED_FILE = "model-00002-of-00004.safetensors"  # holds layers 1 and 4 only


def plan_by_name(name: str):
    from zest_amd.shard import LLAMA_TP
    if name == "stage":
        return stage_plan
    if name == "drop14":
        return {"model.layers.1.*": "drop", "model.layers.4.*": "drop", **LLAMA_TP}
    return name


# ------------------------------------------------------------------------------------------------
# a process group that runs scenarios in sequence
# ------------------------------------------------------------------------------------------------
def _rank_main(rank, world, port, device, cmd_q, res_q):
    import faulthandler
    import sys

    import torch.distributed as dist

    faulthandler.dump_traceback_later(300, exit=True, file=sys.stderr)  # a stack instead of a silent hang
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import zest_amd
        from zest_amd.parallel import swarm_pull_sharded
        from zest_amd.shard import Shard

        if device != "cpu":
            torch.cuda.set_device(torch.device(device))
        while True:
            sc = cmd_q.get()
            if sc is None:
                break
            os.environ.update(sc["env"][rank])
            st: dict = {}
            try:
                sh = Shard(sc.get("as_rank", {}).get(rank, rank), world, plan_by_name(sc.get("plan", "llama-tp")))
                kw = dict(sc.get("kw", {}))
                t0 = time.perf_counter()
                if device == "cpu":  # the public interface
                    got = zest_amd.pull(M.REPO, device="all", p2p=False, dht=False, shard=sh, stats=st, **kw)
                else:  # gloo carries the control traffic, so the device is named
                    peak0 = None
                    if sc.get("measure_memory"):
                        torch.cuda.synchronize()
                        torch.cuda.reset_peak_memory_stats()
                        peak0 = torch.cuda.memory_allocated()
                    got = swarm_pull_sharded(M.REPO, device=device, p2p=False, dht=False, shard=sh, stats=st, **kw)
                    torch.cuda.synchronize()
                    if peak0 is not None:
                        st["shard"]["peak_torch_bytes"] = torch.cuda.max_memory_allocated() - peak0
                st["shard"]["pull_s"] = time.perf_counter() - t0
                tensors = {k: (v.reshape(-1).view(torch.uint8).cpu().numpy().tobytes() if v.numel() else b"",
                               list(v.shape), str(v.dtype), v.is_contiguous(), str(v.device)) for k, v in got.items()}
                del got
                res_q.put((sc["id"], rank, "ok", tensors, st["shard"]))
            except Exception as e:  # noqa: BLE001  (reported; the parent asserts on it)
                res_q.put((sc["id"], rank, type(e).__name__, str(e), None))
                if sc.get("die"):
                    raise
    finally:
        dist.destroy_process_group()


class World:
    """`world` rank processes over gloo, started once; run(scenario) is one collective pull on every
    rank, each rank with its own empty cache roots."""

    def __init__(self, world: int, hub, root, device: str = "cpu"):
        import torch.multiprocessing as mp

        from e2e_util import free_port

        self.world, self.hub, self.root, self.n = world, hub, root, 0
        ctx = mp.get_context("spawn")
        self.res_q = ctx.Queue()
        self.cmd_qs = [ctx.Queue() for _ in range(world)]
        port = free_port()
        self.procs = [ctx.Process(target=_rank_main, args=(r, world, port, device, self.cmd_qs[r], self.res_q))
                      for r in range(world)]
        for p in self.procs:
            p.start()

    def run(self, timeout: float = 240, **scenario):
        """Returns [(status, tensors or message, stats)] by rank."""
        self.n += 1
        sc = dict(scenario, id=self.n,
                  env=[self.hub.env(str(self.root / f"w{self.world}_s{self.n}_r{r}")) for r in range(self.world)])
        for q in self.cmd_qs:
            q.put(sc)
        res = sorted((self.res_q.get(timeout=timeout) for _ in self.procs), key=lambda r: r[1])
        assert [r[0] for r in res] == [self.n] * self.world and [r[1] for r in res] == list(range(self.world)), res
        return [r[2:] for r in res]

    def stop(self, timeout: float = 60):
        """Ends the ranks; returns their exit codes (None: still alive, then killed)."""
        for q, p in zip(self.cmd_qs, self.procs):
            if p.is_alive():
                q.put(None)
        codes = []
        for p in self.procs:
            p.join(timeout=timeout)
            codes.append(p.exitcode)
            if p.is_alive():
                p.kill()
                p.join(10)
        return codes


def assert_exact(tensors: dict, want: dict) -> None:
    """A rank's reported tensors against {name: (bytes, shape)} of the model."""
    assert set(tensors) == set(want)
    for name, (raw, shape) in want.items():
        got_raw, got_shape, _, contiguous, _ = tensors[name]
        assert got_raw == raw and got_shape == shape and contiguous, name
