"""GPU: ops.reuse_chunks (kernel K12, zg_reuse_chunks in csrc/gpu/blake3_flat.hip) against the model
(reuse_model.py): exact bytes at every source x destination misalignment, hashes and sizes at their
rows, and nothing written outside the records' outputs.  No test here provokes a fault: invalid
tables are refused on the host (tests/test_reuse_cpu.py)."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import reuse_model as M
from zest_amd import ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LENS = [0, 1, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 2048, 8191, 65536, 131071, 131072]
ROW_FILL, SIZE_FILL = 0x3C, -7


@pytest.fixture(scope="module")
def pool():
    """Three separate source allocations of exactly their size (torch.empty, no PAD behind them),
    filled once; the host copy is the reference every test slices."""
    rng = np.random.default_rng(5)
    host = [rng.integers(0, 256, n, dtype=np.uint8) for n in (1_500_000, 400_001, 131_072 + 16)]
    dev = []
    for h in host:
        t = torch.empty(len(h), dtype=torch.uint8, device=DEV)
        t.copy_(torch.from_numpy(h))
        dev.append(t)
    torch.cuda.synchronize()
    return host, dev


def _run(pool, picks, lens, dst_mis, rng, rows=None, index=None, check_ranges=True):
    """Records: lens[i] bytes at offset picks[i] = (buffer, start).  Runs the kernel on sentinel-filled
    outputs and compares dst, hashes and sizes with the model over all of their bytes."""
    host, dev = pool
    n = len(lens)
    lens = np.asarray(lens, dtype=np.int64)
    for (b, s), ln in zip(picks, lens):
        assert 0 <= s and s + ln <= len(host[b])
    offs, total = M.layout(lens, dst_mis, rng)
    rows = rows if rows is not None else n + 5
    index = np.asarray(index if index is not None else rng.permutation(rows)[:n])
    dst = torch.full((total,), M.SENTINEL, dtype=torch.uint8, device=DEV)
    hashes = torch.full((rows, 32), ROW_FILL, dtype=torch.uint8, device=DEV)
    sizes = torch.full((rows,), SIZE_FILL, dtype=torch.int64, device=DEV)
    addrs = [dev[b].data_ptr() + s for b, s in picks]
    chunks = [host[b][s:s + ln] for (b, s), ln in zip(picks, lens)]
    want = M.expect(chunks, offs, index, np.full(total, M.SENTINEL, np.uint8), np.full((rows, 32), ROW_FILL, np.uint8),
                    np.full(rows, SIZE_FILL, np.int64))
    ops.reuse_chunks(addrs, lens, dst, offs, hashes, index, sizes, buffers=dev)
    torch.cuda.synchronize()
    got = dst.cpu().numpy()
    bad = np.flatnonzero(got != want[0])
    assert bad.size == 0, f"{bad.size} wrong bytes in dst, first at {bad[0]} (record offsets {offs.tolist()[:8]}...)"
    assert np.array_equal(sizes.cpu().numpy(), want[2])
    hs = hashes.cpu().numpy()
    wrong = np.flatnonzero((hs != want[1]).any(axis=1))
    assert wrong.size == 0, f"hash rows {wrong.tolist()[:8]} differ (lens {lens.tolist()[:8]}...)"
    if check_ranges and n:  # the same hashes from the existing K1 path over the copied bytes
        again = ops.hash_ranges(dst, offs.astype(np.uint64), lens.astype(np.uint32)).cpu().numpy()
        assert np.array_equal(again, want[1][index])
    return dst, hashes, sizes


def test_lengths_from_three_buffers_shuffled(pool):
    """Every edge length, sources drawn from three allocations in shuffled order; one chunk ends at
    the very last byte of an exact-size allocation, one starts at its first byte."""
    host, _ = pool
    rng = np.random.default_rng(1)
    picks = []
    for i, ln in enumerate(LENS):
        b = int(rng.integers(0, 3)) if ln <= len(host[2]) else int(rng.integers(0, 2))
        picks.append((b, int(rng.integers(0, len(host[b]) - ln + 1))))
    picks[LENS.index(131072)] = (2, len(host[2]) - 131072)   # ends with its allocation's last byte
    picks[LENS.index(8191)] = (1, len(host[1]) - 8191)       # ends at an odd last byte
    picks[LENS.index(65536)] = (0, 0)                        # starts with its allocation
    picks[LENS.index(17)] = (1, 0)
    order = rng.permutation(len(LENS))
    _run(pool, [picks[i] for i in order], [LENS[i] for i in order], rng.integers(0, 16, len(LENS)), rng)


@pytest.mark.parametrize("length", [17, 1025])
def test_every_misalignment_pair(pool, length):
    """Source misalignment 0..15 against destination misalignment 0..15: 256 records in one launch."""
    host, dev = pool
    rng = np.random.default_rng(length)
    base = (-dev[0].data_ptr()) % 16  # offset of a 16-byte aligned address in buffer 0
    picks, mis = [], []
    for s in range(16):
        for d in range(16):
            picks.append((0, base + 16 * int(rng.integers(1, 50_000)) + s))
            mis.append(d)
    dst, _, _ = _run(pool, picks, [length] * 256, mis, rng)
    # layout() sets the output offset mod 16; that is the address mod 16 for an aligned dst
    assert dst.data_ptr() % 16 == 0
    assert {((dev[0].data_ptr() + s) % 16, d) for (_, s), d in zip(picks, mis)} == \
        {(s, d) for s in range(16) for d in range(16)}


@pytest.mark.parametrize("leaves", [63, 64, 65])
def test_launch_leaf_totals(pool, leaves):
    """Launches whose leaves fill one wave task less one, exactly, and one more."""
    rng = np.random.default_rng(leaves)
    lens = [20 * 1024 + 5, 30 * 1024, 1, (leaves - 21 - 30 - 1 - 1) * 1024 - 3, 0]  # 21 + 30 + 1 + k + 1 leaves
    assert sum(max(1, -(-ln // 1024)) for ln in lens) == leaves
    picks = [(0, int(rng.integers(0, 1_000_000))) for _ in lens]
    _run(pool, picks, lens, rng.integers(0, 16, len(lens)), rng)


@pytest.mark.parametrize("n", [1, 8, 9])
def test_tree_groups(pool, n):
    """1, 8 and 9 multi-leaf chunks: the tree kernel takes 8 chunks per wave."""
    rng = np.random.default_rng(n)
    lens = [int(x) for x in rng.integers(1025, 40_000, n)]
    picks = [(int(i % 2), int(rng.integers(0, 300_000))) for i in range(n)]
    _run(pool, picks, lens, rng.integers(0, 16, n), rng)


def test_plan_tile_of_one_byte_chunks(pool):
    """1025 one-byte chunks: one more than a plan tile, 64 chunks per wave task."""
    rng = np.random.default_rng(3)
    n = 1025
    picks = [(int(i % 3), int(rng.integers(0, 131_072))) for i in range(n)]
    _run(pool, picks, [1] * n, rng.integers(0, 16, n), rng)


def test_rows_not_named_keep_their_bytes(pool):
    """Non-contiguous, unordered rows in tables far larger than the launch; sizes is optional."""
    host, dev = pool
    rng = np.random.default_rng(4)
    lens = [5000, 1024, 0, 70_000, 1]
    index = [907, 3, 512, 0, 64]
    picks = [(0, 11), (1, 7), (0, 0), (0, 90_001), (2, 5)]
    dst, hashes, sizes = _run(pool, picks, lens, [3, 0, 9, 15, 8], rng, rows=1000, index=index)
    keep = np.setdiff1d(np.arange(1000), index)
    assert (hashes.cpu().numpy()[keep] == ROW_FILL).all() and (sizes.cpu().numpy()[keep] == SIZE_FILL).all()
    h2 = torch.full((1000, 32), ROW_FILL, dtype=torch.uint8, device=DEV)
    offs, total = M.layout(np.asarray(lens), [0] * 5, rng)
    d2 = torch.full((total,), M.SENTINEL, dtype=torch.uint8, device=DEV)
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream())
    ops.reuse_chunks([dev[b].data_ptr() + s for b, s in picks], lens, d2, offs, h2, index, buffers=dev, stream=side)
    side.synchronize()
    assert torch.equal(h2, hashes)
