"""Reference model of the slice scatter (ops.slice_scatter, K15), plain NumPy and byte by byte: no
arithmetic shared with the kernel, with the ops CPU path or with zest_amd.into.

  scatter_model(src, entries)   what a scatter table writes: {dst_addr: bytes}
  check_scatter(...)            run ops.slice_scatter on destinations carved out of canary-filled
                                buffers and compare EVERY byte of every buffer
  case_*(ops, device)           the kernel cases, shared by the CPU-path and the GPU tests
"""
from __future__ import annotations

import numpy as np

import shard_model as M

TILE = 16 << 10  # destination bytes a workgroup of the kernel covers when every block is whole


def scatter_model(src: bytes, entries) -> dict[int, bytes]:
    """entries: (src_off, run_bytes, src_stride, n_runs, dst_addr) -> {dst_addr: output bytes} of the
    entries with any output."""
    out = {}
    for so, rb, st, nr, da in entries:
        b = b"".join(bytes(src[so + r * st:so + r * st + rb]) for r in range(nr))
        if b:
            assert da not in out
            out[da] = bytes(b)
    return out


def canary(n: int, salt: int = 0) -> np.ndarray:
    """Position-dependent filler: neighbours differ, so a byte copied from next door shows too."""
    i = np.arange(n, dtype=np.uint64) + np.uint64(salt)
    c = i * np.uint64(37) + (i >> np.uint64(8)) * np.uint64(101) + np.uint64(11)
    return (c & np.uint64(0xFF)).astype(np.uint8)


def place_source(src: np.ndarray, device, align: int = 0):
    """`src` on `device`, `align` bytes past a 16-byte boundary and ending with the logical range of
    its allocation.  Returns (the allocation, the source view)."""
    import torch

    hold = torch.empty(align + len(src), dtype=torch.uint8, device=device)
    assert hold.data_ptr() % 16 == 0  # torch allocations are at least 64-byte aligned
    s = hold[align:]
    s.copy_(torch.from_numpy(src))
    return hold, s


def check_scatter(ops, device, src: np.ndarray, entries, buf_lens, src_align: int = 0, order=None) -> None:
    """entries: (src_off, run_bytes, src_stride, n_runs, buffer index, offset in that buffer).  Every
    buffer is a separate allocation of buf_lens[k] bytes filled with canary; the table is handed over in
    `order` (default: as given).  After the launch every byte of every buffer is compared: outputs
    equal the model, everything else still holds its canary."""
    import torch

    hold, s = place_source(src, device, src_align)
    bufs, want = [], []
    for k, n in enumerate(buf_lens):
        c = canary(n, 1000 * k)
        t = torch.from_numpy(c.copy()).to(device)
        assert t.data_ptr() % 16 == 0
        bufs.append(t)
        want.append(c.copy())
    absolute = [(so, rb, st, nr, bufs[b].data_ptr() + off) for so, rb, st, nr, b, off in entries]
    where = {bufs[b].data_ptr() + off: (b, off) for _, rb, _, nr, b, off in entries if rb * nr}
    for da, data in scatter_model(src.tobytes(), absolute).items():
        b, off = where[da]
        assert off + len(data) <= buf_lens[b]
        want[b][off:off + len(data)] = np.frombuffer(data, dtype=np.uint8)
    rows = absolute if order is None else [absolute[i] for i in order]
    ops.slice_scatter(s, np.array(rows, dtype=ops.SCATTER_DTYPE), bufs)
    for k, t in enumerate(bufs):
        got = t.cpu().numpy()
        bad = np.flatnonzero(got != want[k])
        assert bad.size == 0, f"buffer {k}: {bad.size} bytes differ, first at offset {int(bad[0])}"
    assert np.array_equal(hold[src_align:].cpu().numpy(), src)  # the source is only read


def _rand(n: int, seed: int = 5) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


# ------------------------------------------------------------------------------------------------
# 1. the alignment grid
# ------------------------------------------------------------------------------------------------
GRID_SIZES = (1, 15, 16, 17, 33, 100)


def grid_layout():
    """One single-run entry per (dst & 15, src & 15, size), all in one buffer, 1-3 canary bytes between
    neighbouring outputs.  The order is found greedily: after each output the gap (1, 2 or 3) is the one
    whose destination alignment has the most combinations left.  Returns (entries, src_len, buf_len)."""
    left = {da: [(sa, n) for n in GRID_SIZES for sa in range(16)] for da in range(16)}
    entries, pos, spos = [], 0, 0
    while any(left.values()):
        g = max((1, 2, 3), key=lambda g: len(left[(pos + g) & 15]))
        assert left[(pos + g) & 15], "the greedy order ran dry"
        pos += g
        sa, n = left[pos & 15].pop()
        spos += (sa - spos) & 15
        entries.append((spos, n, n, 1, 0, pos))
        pos += n
        spos += n
    return entries, spos, pos + 3


def case_alignment_grid(ops, device) -> None:
    entries, src_len, buf_len = grid_layout()
    seen = {(off & 15, so & 15, rb) for so, rb, _, _, _, off in entries}
    assert len(entries) == 16 * 16 * len(GRID_SIZES) == len(seen) == 1536
    ends = sorted((off, off + rb) for _, rb, _, _, _, off in entries)
    assert all(1 <= b[0] - a[1] <= 3 for a, b in zip(ends, ends[1:]))
    check_scatter(ops, device, _rand(src_len), entries, [buf_len])


# ------------------------------------------------------------------------------------------------
# 2. blocks shared by several entries
# ------------------------------------------------------------------------------------------------
SHARED_SIZES = (5, 7, 11, 1, 27, 16, 3)


def case_shared_blocks(ops, device, gap: int) -> None:
    entries, pos, spos = [], 3, 1  # an odd first address
    for n in SHARED_SIZES:
        entries.append((spos, n, n, 1, 0, pos))
        pos += n + gap
        spos += n + 2
    check_scatter(ops, device, _rand(spos, 9), entries, [pos + 20])


# ------------------------------------------------------------------------------------------------
# 3. the run grid of the gather tests, destinations at any alignment
# ------------------------------------------------------------------------------------------------
GRID_STARTS = (0, 1, 8, 15)


def case_run_grid(ops, device, stride: str, start: int) -> None:
    """shard_model.grid_specs (run sizes up to 16 KiB + 2, 1 / 2 / 37 runs): the first output at
    `start` & 15, the next ones 3 bytes after their predecessor, so every entry has another alignment
    and runs that are no multiple of 16 cross inside a vector."""
    laid, src_len, _ = M.lay_out(M.grid_specs(stride))
    entries, pos = [], start
    for so, rb, st, nr, _ in laid:
        entries.append((so, rb, st, nr, 0, pos))
        pos += rb * nr + 3
    check_scatter(ops, device, _rand(src_len, 3), entries, [pos + 16], src_align=5)


# ------------------------------------------------------------------------------------------------
# 4. larger cases
# ------------------------------------------------------------------------------------------------
def case_tiles(ops, device) -> None:
    """An entry over more than three tiles at dst & 15 = 9 as runs of 4099 bytes with stride 4100
    (twelve runs: 4099 does not divide 3 * 16 KiB + 5), and one run of exactly three tiles + 5 bytes."""
    n = 12 * 4099
    assert 3 * TILE < n < 4 * TILE
    one = 3 * TILE + 5
    s2 = 11 * 4100 + 4099 + 7
    entries = [(3, 4099, 4100, 12, 0, 9), (s2, one, one, 1, 1, 16 + 9)]
    check_scatter(ops, device, _rand(s2 + one, 17), entries, [9 + n + 40, 16 + 9 + one + 1], src_align=2)


def case_many_small(ops, device) -> None:
    """300 entries of 7 bytes inside one tile: more than the LDS cache holds."""
    entries = [(11 * i, 7, 7, 1, 0, 5 + 7 * i) for i in range(300)]
    assert 5 + 7 * 300 < TILE
    check_scatter(ops, device, _rand(11 * 300, 23), entries, [5 + 7 * 300 + 30])


# ------------------------------------------------------------------------------------------------
# 5. several allocations, descending table
# ------------------------------------------------------------------------------------------------
def case_three_allocations(ops, device) -> None:
    lens = [4096 + 13, 700, 100_003]
    entries = [(0, 1000, 1000, 1, 0, 17), (1000, 37, 64, 9, 0, lens[0] - 333),  # the second ends with buffer 0
               (2000, 700, 700, 1, 1, 0),                                       # a whole buffer
               (3000, 4099, 4100, 12, 2, 1), (60_000, 50_001, 50_001, 1, 2, 50_002)]  # ends with buffer 2
    assert entries[1][5] + 37 * 9 == lens[0] and entries[4][5] + 50_001 == lens[2]
    src = _rand(60_000 + 50_001, 29)
    check_scatter(ops, device, src, entries, lens, src_align=7)  # ascending within each buffer
    import torch

    # the table in descending address order, whatever order the allocator gave the buffers
    hold, s = place_source(src, device, 7)
    bufs = [torch.from_numpy(canary(n, 1000 * k)).to(device) for k, n in enumerate(lens)]
    rows = sorted(((so, rb, st, nr, bufs[b].data_ptr() + off) for so, rb, st, nr, b, off in entries),
                  key=lambda e: -e[4])
    assert all(a[4] > b[4] for a, b in zip(rows, rows[1:]))
    ops.slice_scatter(s, np.array(rows, dtype=ops.SCATTER_DTYPE), bufs)
    want = [canary(n, 1000 * k) for k, n in enumerate(lens)]
    model = scatter_model(src.tobytes(), rows)
    for so, rb, st, nr, b, off in entries:
        data = model[bufs[b].data_ptr() + off]
        want[b][off:off + len(data)] = np.frombuffer(data, dtype=np.uint8)
    for k, t in enumerate(bufs):
        assert np.array_equal(t.cpu().numpy(), want[k]), f"buffer {k}"


# ------------------------------------------------------------------------------------------------
# 6. nothing to do, 7. refusals
# ------------------------------------------------------------------------------------------------
def case_nothing_to_do(ops, device) -> None:
    """Empty and all-zero tables: every buffer byte keeps its canary (the tests also make a launch,
    were one attempted, raise)."""
    check_scatter(ops, device, _rand(10), [], [64])
    check_scatter(ops, device, _rand(10), [(0, 0, 0, 0, 0, 0), (10, 0, 4, 3, 0, 16), (3, 5, 5, 0, 0, 63)], [64])


def case_refusals(ops, device, pytest) -> None:
    """Every refusal of ops.slice_scatter names the entry and comes before any launch: the buffers
    keep every canary byte."""
    import torch

    hold, src = place_source(_rand(100), device)
    a = torch.from_numpy(canary(64)).to(device)
    b = torch.from_numpy(canary(64, 1000)).to(device)
    A, B = a.data_ptr(), b.data_ptr()
    tab = lambda *e: np.array(list(e), dtype=ops.SCATTER_DTYPE)

    def run(*entries, buffers=(a, b)):
        ops.slice_scatter(src, tab(*entries), list(buffers))

    with pytest.raises(ValueError, match="entry 1.*past the source"):
        run((0, 10, 10, 1, A), (91, 10, 10, 1, B))
    with pytest.raises(ValueError, match="entry 0.*past the source"):
        run((0, 4, 49, 3, A))  # the last run ends at 102
    with pytest.raises(ValueError, match="entry 0.*past the source"):
        run((1 << 63, 2, 1 << 63, 3, A))  # would wrap around 64 bits
    with pytest.raises(ValueError, match="entry 0.*src_stride"):
        run((0, 4, 3, 2, A))
    with pytest.raises(ValueError, match="entry 1.*inside one buffer"):
        run((0, 10, 10, 1, A), (0, 10, 10, 1, B + 55))  # past b's logical end
    with pytest.raises(ValueError, match="entry 0.*inside one buffer"):
        run((0, 10, 10, 1, min(A, B) - 3))  # starts before the first buffer
    with pytest.raises(ValueError, match="entry 0.*inside one buffer"):
        run((0, 10, 10, 1, A), buffers=(b,))  # nobody vouches for a
    with pytest.raises(ValueError, match="entry 0.*inside one buffer"):
        run((0, 10, 10, 1, A), buffers=())
    with pytest.raises(ValueError, match="entry 1.*overlaps entry 0"):
        run((0, 17, 17, 1, A), (20, 4, 4, 1, A + 16))
    with pytest.raises(ValueError, match="entry 2.*overlaps entry 0"):
        run((0, 4, 4, 1, A + 30), (0, 4, 4, 1, B), (0, 2, 2, 4, A + 23))  # its last byte is entry 0's first
    with pytest.raises(ValueError, match="entry 1.*overlaps the source"):
        run((0, 4, 4, 1, A), (0, 4, 4, 1, src.data_ptr() + 96), buffers=(a, hold))
    many = np.broadcast_to(tab((0, 1, 1, 1, A)), (1 << 32,))  # 2^32 entries without their memory
    with pytest.raises(ValueError, match="4294967296 entries"):
        ops.slice_scatter(src, many, [a, b])
    with pytest.raises(ValueError, match="uint8"):
        ops.slice_scatter(src.view(torch.int16), tab(), [a])
    with pytest.raises(ValueError, match="buffer 1 is on"):
        ops.slice_scatter(src, tab(), [a, torch.empty(4, dtype=torch.uint8, device="meta")])
    assert np.array_equal(a.cpu().numpy(), canary(64)) and np.array_equal(b.cpu().numpy(), canary(64, 1000))
    # all legal, to the last byte of a
    run((90, 10, 10, 1, A + 54), (0, 4, 48, 3, B + 1), (100, 0, 0, 0, 0), (0, 1, 1, 16, B + 13))
    assert a.cpu().numpy()[54:].tobytes() == src.cpu().numpy()[90:].tobytes()
