"""GPU: the several-source slice gather (csrc/gpu/shard_peers.hip, ops.slice_gather_peers) against the
plain-NumPy model byte for byte, canaries around the arena and in every gap; then the collective
sharded pull rehearsed with every rank on the one GPU (gloo for control, as test_gpu_ipc.py): the
mapped exchange, the cross-check of both exchanges, the send exchange on device tensors and the
memory bound of one rank."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import shard_collective_util as U
import shard_model as M
from e2e_util import free_port
from zest_amd import ops
from zest_amd.shard import Shard, plan_file
from zest_amd.testing import FakeHub

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TILE = 16 << 10  # arena bytes per tile of the kernel


# ------------------------------------------------------------------------------------------------
# kernel
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 3, 16])
@pytest.mark.parametrize("stride", list(M.STRIDES))
def test_run_grid_dealt_over_sources(stride, k):
    """run_bytes x n_runs dealt over k sources, each source at its own offset past a 16-byte boundary."""
    parts, arena = U.deal(M.grid_specs(stride), k)
    for shift in (0, 7):
        U.check_gather_peers(ops, DEV, parts, arena, aligns=[(5 * s + 3 + shift) % 16 for s in range(k)])


def test_source_boundaries_inside_one_tile():
    specs = [(16, 1, 16), (17, 2, 19), (48, 1, 48), (3, 5, 7), (31, 1, 31), (16, 3, 16), (40, 1, 44), (24, 2, 24),
             (33, 1, 33)]
    parts, arena = U.deal(specs, 3, dst_step=16)
    assert arena < TILE and all(len(e) == 3 for _, e in parts)
    U.check_gather_peers(ops, DEV, parts, arena, aligns=[1, 15, 6])


def test_more_entries_than_the_cache_next_to_one_large_entry():
    small, small_len, small_end = M.lay_out([(16, 1, 16)] * 300, dst_step=16)
    assert small_end == 300 * 16 < TILE  # more than kCache (256) entries in the first tile
    big_rb = (1 << 20) + 2
    parts = [(U.source_bytes(small_len, 1), small),
             (U.source_bytes(big_rb + 5, 2), [(5, big_rb, big_rb, 1, small_end)])]  # shares the first tile
    U.check_gather_peers(ops, DEV, parts, small_end + big_rb, aligns=[3, 11])
    # the large entry first: the small source's entries then start in the middle of a later tile
    big_first = [(parts[1][0], [(5, big_rb, big_rb, 1, 0)]),
                 (parts[0][0], [(so, rb, st, nr, do + big_rb + 14) for so, rb, st, nr, do in small])]
    U.check_gather_peers(ops, DEV, big_first, big_rb + 14 + small_end, aligns=[0, 9])


@pytest.mark.parametrize("max_blocks", [3, 0], ids=["one-block-per-source", "default-cap"])
def test_blocks_loop_over_their_sources_tiles(max_blocks):
    parts, arena = U.deal([(50_001, 3, 50_008), (24, 1, 24), (70_000, 2, 70_001), (1 << 17, 1, 1 << 17),
                           (33, 37, 40), (90_001, 1, 90_001)], 3)
    assert all(sum(rb * nr for _, rb, _, nr, _ in e) > 4 * TILE for _, e in parts)  # several tiles per source
    U.check_gather_peers(ops, DEV, parts, arena, max_blocks=max_blocks)


def test_all_zero_and_empty_tables_launch_nothing():
    U.check_gather_peers(ops, DEV, [(U.source_bytes(10, 1), [(0, 0, 0, 0, 0), (10, 0, 4, 3, 16)]),
                                    (U.source_bytes(10, 2), [(3, 5, 5, 0, 32)])], 48)
    U.check_gather_peers(ops, DEV, [(U.source_bytes(10, 1), []), (U.source_bytes(0, 2), [])], 0)
    U.check_gather_peers(ops, DEV, [], 0)


def test_refuses_before_launching():
    U.check_refusals(ops, DEV)
    src = torch.zeros(100, dtype=torch.uint8, device=DEV)
    dst = torch.zeros(80, dtype=torch.uint8, device=DEV)
    tab = lambda *e: np.array(list(e), dtype=ops.SLICE_DTYPE)
    with pytest.raises(ValueError, match="source 1 entry 0.*past the arena"):
        ops.slice_gather_peers([src, src], [tab(), tab((0, 5, 5, 1, 80))], dst)
    with pytest.raises(ValueError, match="16-byte aligned"):
        ops.slice_gather_peers([src], [tab((0, 5, 5, 1, 0))], dst[8:])
    with pytest.raises(ValueError, match="source 1 is on cpu"):
        ops.slice_gather_peers([src, src.cpu()], [tab((0, 5, 5, 1, 0)), tab()], dst)
    assert not dst.any()
    s = torch.cuda.Stream(DEV)  # an explicit stream
    src.fill_(7)
    s.wait_stream(torch.cuda.current_stream(DEV))
    ops.slice_gather_peers([src, src], [tab((3, 5, 9, 4, 16)), tab((1, 3, 3, 1, 48))], dst, stream=s)
    s.synchronize()
    assert dst.cpu().tolist() == [0] * 16 + [7] * 20 + [0] * 12 + [7] * 3 + [0] * 29


# ------------------------------------------------------------------------------------------------
# end to end: every rank on the one GPU, gloo for control; at most 4 rank processes at a time
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    files = M.build_repo()
    hub = FakeHub(policy="auto", max_xorb_bytes=1 << 20)
    hub.start()
    root = tmp_path_factory.mktemp("gpucollective")
    out = {"files": files}
    mp = pytest.MonkeyPatch()
    mp.setenv("ZEST_LISTEN_PORT", str(free_port()))
    w = None
    try:
        hub.add_repo(M.REPO, files, xet_suffixes=(".safetensors",))
        w = U.World(2, hub, root, device=DEV)
        out["mapped"] = w.run(kw={"exchange": "mapped"})
        out["cross"] = w.run(kw={"cross_check": True})
        assert w.stop() == [0, 0]
        w = U.World(4, hub, root, device=DEV)
        out["send"] = w.run(kw={"exchange": "send"})
        largest = max(len(files[p]) for p in M.FILES)
        out["memory"] = w.run(kw={"scratch_bytes": largest}, measure_memory=True)
        assert w.stop() == [0] * 4
        yield out
    finally:
        if w is not None:
            w.stop()
        mp.undo()
        hub.stop()


def _exact(runs, key, world):
    res = runs[key]
    assert [r[0] for r in res] == ["ok"] * world, res
    for rank, (_, tensors, _) in enumerate(res):
        U.assert_exact(tensors, M.expected_shard(runs["files"], rank, world))
        assert all(t[4].startswith("cuda") for t in tensors.values())


def test_mapped_exchange_two_ranks(runs):
    _exact(runs, "mapped", 2)
    for _, _, st in runs["mapped"]:
        assert st["exchange"] == "mapped" and st["rounds"] >= 1 and st["received_bytes"] > 0
        print(f"mapped world 2: pull {st['pull_s']:.3f} s, gather per round {st['round_gather_s']}")


def test_cross_check_two_ranks(runs):
    _exact(runs, "cross", 2)
    for _, _, st in runs["cross"]:
        assert st["exchange"] == "mapped" and st["cross_checked_bytes"] == st["kept_bytes"] > 0


def test_send_exchange_four_ranks_on_device_tensors(runs):
    _exact(runs, "send", 4)
    for _, _, st in runs["send"]:
        assert st["exchange"] == "send"
        print(f"send world 4: pull {st['pull_s']:.3f} s, gather per round {st['round_gather_s']}")


def test_memory_of_one_rank_stays_bounded(runs):
    """scratch_bytes = the largest file.  Peak torch memory over the pull stays within this rank's
    arenas + ops.PAD + 256 bytes per tensor; the VMM scratch lies outside torch's allocator and is
    reported in scratch_bytes.  A replicated pull (every file resident) cannot meet the bound."""
    files = runs["files"]
    sizes = [len(files[p]) for p in M.FILES]
    _exact(runs, "memory", 4)
    for rank, (_, _, st) in enumerate(runs["memory"]):
        plans = [plan_file(*M.header(files[p]), Shard(rank, 4), len(files[p])) for p in M.FILES]
        bound = sum(p.arena_bytes for p in plans) + ops.PAD + 256 * sum(len(p.tensors) for p in plans)
        assert bound < sum(sizes), (bound, sum(sizes))  # else it could not tell this pull from a replicated one
        print(f"rank {rank}: peak {st['peak_torch_bytes']} bound {bound} files {sum(sizes)} "
              f"scratch {st['scratch_bytes']} exchange {st['exchange']} pull {st['pull_s']:.3f} s")
        assert st["exchange"] == "mapped" and 0 < st["scratch_bytes"] <= max(sizes) + 2 * ops.PAD
        assert st["peak_torch_bytes"] <= bound, (rank, st["peak_torch_bytes"], bound)
