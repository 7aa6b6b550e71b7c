"""GPU: the slice-gather kernel (csrc/gpu/shard.hip, ops.slice_gather) against the plain-NumPy model
byte for byte, canaries around the arena and in every padding gap, the source ending with its
allocation's logical range; then pull(device="cuda:0", shard=...) end to end over a FakeHub against
the CPU sharded pull, the scratch reuse across groups, and the memory bound of a sharded pull."""
from __future__ import annotations

import json
import struct

import numpy as np
import pytest
import torch

import shard_model as M
import zest_amd
from e2e_util import free_port
from zest_amd import ops
from zest_amd.shard import Shard, plan_file
from zest_amd.testing import FakeHub

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _src(n, seed=5):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


@pytest.mark.parametrize("stride", list(M.STRIDES))
def test_run_grid_at_every_source_alignment(stride):
    """run_bytes x n_runs, each tensor of the launch at its own source alignment, and the whole
    source at each of the 16 alignments (largest launch: 5.6 MB of source, 0.7 MB of output)."""
    entries, src_len, arena = M.lay_out(M.grid_specs(stride))
    src = _src(src_len)
    for align in range(16):
        M.check_gather(ops, DEV, src, entries, arena, align)


@pytest.mark.parametrize("specs,step", [
    ([(50_001, 3, 50_008)], 256),                                     # one tensor over ten output tiles
    ([(1 << 20, 1, 1 << 20), (3, 5, 11)], 256),                       # a whole tensor, 64 full tiles
    ([(24, 1, 24)] * 600, 32),                                        # 512 tensors in a tile: past the LDS cache
    ([(24, 1, 24)] * 150, 16 << 10),                                  # one tiny tensor per tile
    ([(0, 5, 0), (7, 0, 9), (33, 2, 40), (0, 0, 0), (5, 3, 5), (9, 0, 9), (0, 1, 4)], 16),  # zero sizes
    ([(0, 1, 0)] * 300 + [(40, 2, 41)] + [(0, 0, 0)] * 300, 16),      # zero-size entries fill the cache
    ([(17, 1, 17)], 256),                                             # a single entry
    ([(1, 1, 1)], 256)], ids=["tiles", "whole", "many", "sparse", "zeros", "zerocache", "single", "byte"])
def test_table_shapes(specs, step):
    entries, src_len, arena = M.lay_out(specs, dst_step=step)
    for align in (0, 9):
        M.check_gather(ops, DEV, _src(src_len), entries, arena, align)


def test_all_zero_and_empty_tables_launch_nothing():
    M.check_gather(ops, DEV, _src(10), [(0, 0, 0, 0, 0), (10, 0, 4, 3, 16)], 32)
    M.check_gather(ops, DEV, _src(10), [], 0)


@pytest.mark.parametrize("action", [0, 1, 2, (1, 1, 6), None], ids=["dim0", "middle", "last", "range", "whole"])
@pytest.mark.parametrize("dtype,pad", [("BF16", 3), ("F32", 0), ("U8", 7)])
def test_dims_of_a_3d_tensor(action, dtype, pad):
    """plan_file + kernel against the model's frombuffer/reshape/slice, data section at an odd start."""
    shape, world, rank = [6, 9, 42], 3, 2
    n = int(np.prod(shape)) * M.ITEMSIZE[dtype]
    head = json.dumps({"w": {"dtype": dtype, "shape": shape, "data_offsets": [5, 5 + n]}}).encode() + b" " * pad
    data = struct.pack("<Q", len(head)) + head + _src(5 + n, seed=n).tobytes()
    start, meta = M.header(data)
    plan = plan_file(start, meta, Shard(rank, world, {"w": action}), len(data))
    hold = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to(DEV)
    arena = ops.padded_empty(plan.arena_bytes, DEV)
    ops.slice_gather(hold, plan.table, arena)
    got = plan.views(arena)["w"]
    if action is None:
        want, wshape = M.tensor_slice(data, "w")
    elif isinstance(action, tuple):
        want, wshape = M.tensor_slice(data, "w", *action)
    else:
        want, wshape = M.tensor_slice(data, "w", action, *M.chunk_range(shape[action], rank, world))
    assert list(got.shape) == wshape and got.is_contiguous() and got.device.type == "cuda"
    assert got.cpu().reshape(-1).view(torch.uint8).numpy().tobytes() == want


def test_refuses_before_launching():
    src = torch.zeros(100, dtype=torch.uint8, device=DEV)
    dst = torch.zeros(80, dtype=torch.uint8, device=DEV)
    tab = lambda *e: np.array(list(e), dtype=ops.SLICE_DTYPE)
    with pytest.raises(ValueError, match="entry 0.*past the source"):
        ops.slice_gather(src, tab((96, 5, 5, 1, 0)), dst)
    with pytest.raises(ValueError, match="entry 0.*past the arena"):
        ops.slice_gather(src, tab((0, 5, 5, 1, 80)), dst)
    with pytest.raises(ValueError, match="16-byte aligned"):
        ops.slice_gather(src, tab((0, 5, 5, 1, 0)), dst[8:])
    with pytest.raises(ValueError, match="share a device"):
        ops.slice_gather(src, tab((0, 5, 5, 1, 0)), dst.cpu())
    s = torch.cuda.Stream(DEV)  # an explicit stream
    src.fill_(7)
    s.wait_stream(torch.cuda.current_stream(DEV))
    ops.slice_gather(src, tab((3, 5, 9, 4, 16)), dst, stream=s)
    s.synchronize()
    assert dst.cpu().tolist() == [0] * 16 + [7] * 20 + [0] * 44


# ------------------------------------------------------------------------------------------------
# end to end
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def e2e(tmp_path_factory):
    files = M.build_repo()
    hub = FakeHub(policy="auto", max_xorb_bytes=1 << 20)
    hub.start()
    mp = pytest.MonkeyPatch()
    try:
        hub.add_repo(M.REPO, files, xet_suffixes=(".safetensors",))
        mp.setenv("ZEST_LISTEN_PORT", str(free_port()))
        for k, v in hub.env(str(tmp_path_factory.mktemp("cpushard"))).items():
            mp.setenv(k, v)
        cpu = [zest_amd.pull(M.REPO, device="cpu", p2p=False, dht=False, shard=(r, M.WORLD)) for r in range(M.WORLD)]
        for k, v in hub.env(str(tmp_path_factory.mktemp("gpushard"))).items():  # empty caches for the device pulls
            mp.setenv(k, v)
        yield {"files": files, "cpu": cpu}
    finally:
        mp.undo()
        hub.stop()


def _same(got: dict, want: dict) -> None:
    assert set(got) == set(want)
    for name, t in got.items():
        w = want[name]
        assert t.device.type == "cuda" and t.dtype == w.dtype and t.shape == w.shape and t.is_contiguous(), name
        assert torch.equal(t.cpu().reshape(-1).view(torch.uint8), w.reshape(-1).view(torch.uint8)), name


@pytest.mark.parametrize("rank", range(M.WORLD))
def test_e2e_device_equals_cpu_sharded_pull(e2e, rank):
    st = {}
    got = zest_amd.pull(M.REPO, device=DEV, p2p=False, dht=False, shard=(rank, M.WORLD), stats=st)
    _same(got, e2e["cpu"][rank])
    s = st["shard"]
    assert s["groups"] == 1 and s["skipped_files"] == [] and s["gather_s"] > 0
    assert s["file_bytes"] == sum(len(e2e["files"][p]) for p in M.FILES)
    assert s["kept_bytes"] == sum(t.numel() * t.element_size() for t in got.values())


def test_e2e_groups_reuse_the_scratch_and_memory_stays_bounded(e2e):
    """scratch_bytes = the largest file: every file is a group of its own, the largest first, and each
    later, smaller file lands in the slot the one before it was gathered from.  Peak torch memory over
    the pull stays within arenas + scratch + one file (+ ops.PAD and 256 bytes per tensor), a bound
    that an unsharded pull of this repository (every file resident) cannot meet."""
    files, rank = e2e["files"], 1
    sizes = [len(files[p]) for p in M.FILES]
    largest = max(sizes)
    assert sizes[0] == largest
    sh = Shard(rank, M.WORLD)
    plans = [plan_file(*M.header(files[p]), sh, len(files[p])) for p in M.FILES]
    n_tensors = sum(len(p.tensors) for p in plans)
    scratch = -(-largest // ops.PAD) * ops.PAD + ops.PAD  # the slot of the largest file
    bound = sum(p.arena_bytes for p in plans) + scratch + largest + ops.PAD + 256 * n_tensors
    assert bound < sum(sizes), (bound, sum(sizes))  # else the bound could not tell a sharded pull from a full one
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(DEV)
    base = torch.cuda.memory_allocated(DEV)
    st = {}
    got = zest_amd.pull(M.REPO, device=DEV, p2p=False, dht=False, shard=sh, scratch_bytes=largest, stats=st)
    peak = torch.cuda.max_memory_allocated(DEV) - base
    print(f"peak {peak} bound {bound} files {sum(sizes)} scratch {st['shard']['scratch_bytes']}")
    assert st["shard"]["groups"] == len(M.FILES) and st["shard"]["scratch_bytes"] == scratch
    _same(got, e2e["cpu"][rank])
    assert peak <= bound, (peak, bound)
