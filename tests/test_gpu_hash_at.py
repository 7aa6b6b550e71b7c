"""GPU: ops.hash_chunks_at (zg_hash_chunks_at in csrc/gpu/blake3_flat.hip, K12 without the copy)
against _core.chunk_hash of the same bytes: every edge length at every misalignment, chunks that end
with an exactly sized allocation, shuffled rows, untouched rows and sources.  No test here provokes
a fault: tables the kernel could not run safely are refused on the host, before any launch."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from zest_amd import _core, ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LENS = [0, 1, 63, 64, 65, 1023, 1024, 1025, 65536, 131072]
ROW_FILL, SIZE_FILL = 0x3C, -7


@pytest.fixture(scope="module")
def pool():
    """Two allocations of exactly their size (torch.empty: no pad behind them) and the host copies
    every test slices."""
    rng = np.random.default_rng(14)
    host = [rng.integers(0, 256, n, dtype=np.uint8) for n in (3_210_000, 131_072 + 15)]
    dev = []
    for h in host:
        t = torch.empty(len(h), dtype=torch.uint8, device=DEV)
        t.copy_(torch.from_numpy(h))
        dev.append(t)
    torch.cuda.synchronize()
    return host, dev


def _run(pool, picks, lens, index, rows):
    host, dev = pool
    hashes = torch.full((rows, 32), ROW_FILL, dtype=torch.uint8, device=DEV)
    sizes = torch.full((rows,), SIZE_FILL, dtype=torch.int64, device=DEV)
    want_h = np.full((rows, 32), ROW_FILL, np.uint8)
    want_s = np.full(rows, SIZE_FILL, np.int64)
    for (b, s), ln, r in zip(picks, lens, index):
        assert 0 <= s and s + ln <= len(host[b])
        want_h[r] = np.frombuffer(_core.chunk_hash(host[b][s:s + ln].tobytes()), dtype=np.uint8)
        want_s[r] = ln
    ops.hash_chunks_at([dev[b].data_ptr() + s for b, s in picks], lens, hashes, index, sizes, buffers=dev)
    torch.cuda.synchronize()
    hs = hashes.cpu().numpy()
    wrong = np.flatnonzero((hs != want_h).any(axis=1))
    assert wrong.size == 0, f"hash rows {wrong.tolist()[:8]} differ"
    assert np.array_equal(sizes.cpu().numpy(), want_s)
    for h, d in zip(host, dev):  # the sources are only read
        assert np.array_equal(d.cpu().numpy(), h)


def test_every_length_at_every_misalignment_rows_shuffled(pool):
    """160 records in one launch, laid out back to back in the large allocation so that each starts at
    its misalignment; rows in shuffled order among rows no record names."""
    _, dev = pool
    rng = np.random.default_rng(2)
    picks, lens, at = [], [], 0
    for ln in LENS:
        for mis in range(16):
            at = (at + 15) // 16 * 16 + mis
            assert (dev[0].data_ptr() + at) % 16 == mis
            picks.append((0, at))
            lens.append(ln)
            at += ln
    rows = len(lens) + 9
    _run(pool, picks, lens, rng.permutation(rows)[:len(lens)], rows)


def test_chunks_that_end_with_their_allocation(pool):
    """Chunks ending on the last byte of an exactly sized allocation, at every length that fits and
    the whole allocation's first byte; nothing behind the last byte is the kernel's to read."""
    host, _ = pool
    picks = [(1, len(host[1]) - ln) for ln in LENS] + [(0, len(host[0]) - ln) for ln in LENS] + [(1, 0)]
    lens = LENS + LENS + [131072]
    _run(pool, picks, lens, np.arange(len(lens))[::-1].copy(), len(lens))


def test_small_exact_storages():
    """A chunk that is the whole of a torch.empty(k) storage, k down to one byte."""
    rng = np.random.default_rng(3)
    host = [rng.integers(0, 256, k, dtype=np.uint8) for k in (1, 3, 4, 5, 4095, 4096, 8193)]
    dev = [torch.from_numpy(h).to(DEV) for h in host]
    hashes = torch.zeros((len(host), 32), dtype=torch.uint8, device=DEV)
    ops.hash_chunks_at([d.data_ptr() for d in dev], [len(h) for h in host], hashes, np.arange(len(host)), buffers=dev)
    got = hashes.cpu().numpy()
    for i, h in enumerate(host):
        assert bytes(got[i]) == _core.chunk_hash(h.tobytes())


def test_two_launches_share_the_scratch(pool, monkeypatch):
    """The 1 GiB launch cut, exercised with a small limit: the records before and after the cut are
    all hashed into their rows."""
    monkeypatch.setattr(ops, "REUSE_LAUNCH_BYTES", 300_000)
    picks = [(0, 7 + 100_003 * i) for i in range(12)]
    lens = [100_000 - 1000 * i for i in range(12)]
    _run(pool, picks, lens, np.arange(12), 12)


def test_refusals(pool):
    host, dev = pool
    hashes = torch.full((4, 32), ROW_FILL, dtype=torch.uint8, device=DEV)
    a = dev[0].data_ptr()
    two = [dev[0][:1000], dev[0][1000:2000]]
    with pytest.raises(ValueError, match="record 1: chunk .* lies outside every buffer"):
        ops.hash_chunks_at([a, a + len(host[0]) - 10], [10, 11], hashes, [0, 1], buffers=dev)
    with pytest.raises(ValueError, match="record 0: chunk .* lies outside every buffer"):
        ops.hash_chunks_at([a + 990], [20], hashes, [0], buffers=two)  # spans two adjacent buffers
    with pytest.raises(ValueError, match="record 0: chunk .* lies outside every buffer"):
        ops.hash_chunks_at([a], [10], hashes, [0], buffers=[])
    with pytest.raises(ValueError, match="record 1: index 2 is also record 0's"):
        ops.hash_chunks_at([a, a + 10], [10, 10], hashes, [2, 2], buffers=dev)
    with pytest.raises(ValueError, match=r"record 0: index 4 is past the table \(4 rows\)"):
        ops.hash_chunks_at([a], [10], hashes, [4], buffers=dev)
    with pytest.raises(ValueError, match="record 0: len 131073 is over the chunk maximum of 131072 bytes"):
        ops.hash_chunks_at([a], [131073], hashes, [0], buffers=dev)
    with pytest.raises(ValueError, match="buffer 0 is on cpu"):
        ops.hash_chunks_at([a], [10], hashes, [0], buffers=[torch.zeros(10, dtype=torch.uint8)])
    torch.cuda.synchronize()
    assert (hashes.cpu().numpy() == ROW_FILL).all()  # nothing was launched
