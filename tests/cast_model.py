"""Reference model of the converting slice scatter (ops.slice_scatter_cast, K16): the six float
conversions as integer bit arithmetic on NumPy unsigned arrays, straight from the IEEE rule (decompose,
renormalise, round to nearest even once, re-encode).  No torch, no astype between float types, no
arithmetic shared with the kernel, with the ops CPU path or with zest_amd.into.

  convert(bits, src, dst)          bit patterns of one format -> bit patterns of another
  is_nan(bits, fmt)                which patterns are NaNs
  cast_scatter_model(src, entries) what a cast table writes: {dst_addr: bytes}
  check_cast(...)                  run ops.slice_scatter_cast on destinations carved out of canary-filled
                                   buffers and compare EVERY byte of every buffer: bit for bit, except
                                   where the SOURCE element is a NaN, where a NaN is required
  values(src, dst)                 the value set of a conversion
  case_*(ops, device)              the kernel cases, shared by the CPU-path and the GPU tests
"""
from __future__ import annotations

import functools

import numpy as np

import shard_model as M
from scatter_model import canary, place_source

TILE = 16 << 10  # destination bytes a workgroup of the kernel covers when every block is whole
FORMATS = {"F32": (8, 23), "F16": (5, 10), "BF16": (8, 7)}  # exponent bits, stored significand bits
ITEM = {"F32": 4, "F16": 2, "BF16": 2}
PAIRS = (("F32", "BF16"), ("F32", "F16"), ("BF16", "F32"), ("F16", "F32"), ("BF16", "F16"), ("F16", "BF16"))
U = np.uint64


def _utype(fmt: str):
    return np.dtype("<u4") if ITEM[fmt] == 4 else np.dtype("<u2")


def is_nan(bits: np.ndarray, fmt: str) -> np.ndarray:
    eb, mb = FORMATS[fmt]
    b = bits.astype(U)
    return (((b >> U(mb)) & U((1 << eb) - 1)) == U((1 << eb) - 1)) & ((b & U((1 << mb) - 1)) != U(0))


def convert(bits: np.ndarray, src: str, dst: str) -> np.ndarray:
    """value = sig * 2^ex exactly; the destination's quantum at that magnitude is 2^qe; the result is
    sig * 2^(ex - qe) rounded to an integer, ties to even, added onto the exponent field below it, so a
    carry out of the significand steps the exponent and a carry out of the largest finite gives
    infinity.  A NaN gives the destination's quiet NaN."""
    se, sm = FORMATS[src]
    de, dm = FORMATS[dst]
    b = bits.astype(U)
    sign = b >> U(se + sm)
    e = ((b >> U(sm)) & U((1 << se) - 1)).astype(np.int64)
    m = b & U((1 << sm) - 1)
    top = (1 << se) - 1
    nan, inf = (e == top) & (m != U(0)), (e == top) & (m == U(0))
    sig = np.where(e == 0, m, m | U(1 << sm))                      # subnormals have no hidden bit
    ex = np.where(e == 0, 1, e) - ((1 << (se - 1)) - 1) - sm       # exponent of sig's unit
    p = np.zeros(b.shape, dtype=np.int64)                          # index of sig's highest set bit
    for k in range(1, sm + 1):
        p += (sig >> U(k)) != U(0)
    dbias = (1 << (de - 1)) - 1
    biased = np.maximum(p + ex + dbias, 1)                         # destination exponent field (1: also subnormal)
    qe = biased - dbias - dm
    sh = qe - ex                                                   # right shift of sig (negative: left)
    right = np.clip(sh, 1, 40).astype(U)
    q = sig >> right
    rem, half = sig & ((U(1) << right) - U(1)), U(1) << (right - U(1))
    q = q + ((rem > half) | ((rem == half) & ((q & U(1)) == U(1)))).astype(U)
    full = np.where(sh > 0, q, sig << np.clip(-sh, 0, 40).astype(U))  # with the hidden bit when normal
    out = np.where(full >= U(1 << dm), (biased - 1).astype(U) << U(dm), U(0)) + full
    dtop = U(((1 << de) - 1) << dm)
    out = np.where(inf | (out >= dtop), dtop, out)
    out = np.where(sig == U(0), U(0), out)
    out = np.where(nan, dtop | U(1 << (dm - 1)), out)
    return (out | (sign << U(de + dm))).astype(_utype(dst))


def _entry(src: bytes, so, rb, st, nr, pair):
    """(converted bytes, per-output-element NaN flags) of one entry."""
    raw = b"".join(bytes(src[so + r * st:so + r * st + rb]) for r in range(nr))
    bits = np.frombuffer(raw, dtype=_utype(pair[0]))
    return convert(bits, *pair).tobytes(), is_nan(bits, pair[0])


def cast_scatter_model(src: bytes, entries) -> dict[int, bytes]:
    """entries: (src_off, run_bytes, src_stride, n_runs, dst_addr, (stored dtype, destination dtype))
    -> {dst_addr: output bytes} of the entries with any output."""
    out = {}
    for so, rb, st, nr, da, pair in entries:
        b, _ = _entry(src, so, rb, st, nr, pair)
        if b:
            assert da not in out
            out[da] = b
    return out


def table(ops, rows) -> np.ndarray:
    """(src_off, run_bytes, src_stride, n_runs, dst_addr, pair) rows as an ops.CAST_DTYPE table."""
    return np.array([(so, rb, st, nr, da, ops.CAST_KINDS[pair]) for so, rb, st, nr, da, pair in rows],
                    dtype=ops.CAST_DTYPE)


def check_cast(ops, device, src: np.ndarray, entries, buf_lens, src_align: int = 0, order=None):
    """entries: (src_off, run_bytes, src_stride, n_runs, buffer index, offset in that buffer, pair).
    Every buffer is a separate allocation of buf_lens[k] bytes filled with canary; the table is handed
    over in `order` (default: as given; "descending": by falling address).  After the launch every byte
    of every buffer is compared: outputs equal the model (a NaN where the source element is one), everything else still holds its
    canary.  Returns [(buffer bytes, mask of the bytes that hold a NaN)], for comparing two devices."""
    import torch

    hold, s = place_source(src, device, src_align)
    bufs, want, loose = [], [], []
    for k, n in enumerate(buf_lens):
        c = canary(n, 1000 * k)
        t = torch.from_numpy(c.copy()).to(device)
        assert t.data_ptr() % 16 == 0
        bufs.append(t)
        want.append(c.copy())
        loose.append(np.zeros(n, dtype=bool))
    nan_at = []  # (buffer, offset, destination dtype, element count): outputs with NaNs to look at
    raw = src.tobytes()
    for so, rb, st, nr, b, off, pair in entries:
        data, nans = _entry(raw, so, rb, st, nr, pair)
        if not data:
            continue
        assert off + len(data) <= buf_lens[b]
        want[b][off:off + len(data)] = np.frombuffer(data, dtype=np.uint8)
        if nans.any():
            loose[b][off:off + len(data)] = np.repeat(nans, ITEM[pair[1]])
            nan_at.append((b, off, pair[1], len(nans), nans))
    rows = [(so, rb, st, nr, bufs[b].data_ptr() + off, pair) for so, rb, st, nr, b, off, pair in entries]
    if order == "descending":  # by address, whatever order the allocator gave the buffers
        rows = sorted(rows, key=lambda e: -e[4])
        assert all(a[4] > b[4] for a, b in zip(rows, rows[1:]))
    elif order is not None:
        rows = [rows[i] for i in order]
    ops.slice_scatter_cast(s, table(ops, rows), bufs)
    got = [t.cpu().numpy() for t in bufs]
    for k in range(len(bufs)):
        bad = np.flatnonzero((got[k] != want[k]) & ~loose[k])
        assert bad.size == 0, f"buffer {k}: {bad.size} bytes differ, first at offset {int(bad[0])}"
    for b, off, fmt, n, nans in nan_at:
        elems = np.frombuffer(got[b][off:off + n * ITEM[fmt]].tobytes(), dtype=_utype(fmt))
        assert is_nan(elems, fmt)[nans].all(), f"buffer {b}, output at {off}: a NaN came out as a number"
    assert np.array_equal(hold[src_align:].cpu().numpy(), src)  # the source is only read
    return list(zip(got, loose))


# ------------------------------------------------------------------------------------------------
# value sets: the smallest that hit every rounding case
# ------------------------------------------------------------------------------------------------
BF16_LOW_HALVES = (0, 1, 0x7FFF, 0x8000, 0x8001, 0xFFFF)


@functools.lru_cache(maxsize=None)
def values(src: str, dst: str) -> np.ndarray:
    """Bit patterns of `src` to convert to `dst`.  16-bit sources: all 65,536.  F32 -> BF16: every bf16
    pattern with six low halves (ties at even and odd, carries into the exponent and into infinity,
    subnormals).  F32 -> F16: every finite f16 value v with a finite successor w, the midpoint of v and
    w and its two f32 neighbours; the overflow threshold and the smallest ties; and the F32 -> BF16 set
    for far underflow and overflow."""
    if src != "F32":
        return np.arange(1 << 16, dtype=np.uint32).astype("<u2")
    h = np.arange(1 << 16, dtype=np.uint32) << np.uint32(16)
    coarse = np.concatenate([h | np.uint32(low) for low in BF16_LOW_HALVES])
    if dst == "BF16":
        return coarse.astype("<u4")
    mag = np.arange(0x7BFF, dtype=np.uint32)  # finite, with a finite successor
    v16 = np.concatenate([mag, mag | np.uint32(0x8000)])
    v = convert(v16, "F16", "F32")  # widening is exact
    w = convert(v16 + np.uint32(1), "F16", "F32")
    mid = ((v.view(np.float32) + w.view(np.float32)) * np.float32(0.5)).view(np.uint32)  # 12 significant bits: exact
    edge = np.array([0x477FEFFF, 0x477FF000, 0x33000000, 0x33000001, 0x33800000], dtype=np.uint32)
    return np.concatenate([v, mid, mid - np.uint32(1), mid + np.uint32(1), edge, edge | np.uint32(1 << 31),
                           coarse]).astype("<u4")


@functools.lru_cache(maxsize=None)
def _values_source():
    """The six value sets back to back as one source: (bytes, [(offset, byte length, pair)])."""
    parts, where, pos = [], [], 0
    for pair in PAIRS:
        raw = values(*pair).tobytes()
        where.append((pos, len(raw), pair))
        parts.append(raw)
        pos += len(raw) + 6  # the next set starts at another alignment
        parts.append(b"\0" * 6)
    return np.frombuffer(b"".join(parts), dtype=np.uint8), where


def case_values(ops, device, src_align: int) -> None:
    """One entry per kind over its value set in one launch, destinations 16-byte aligned, the source
    `src_align` bytes past a 16-byte boundary."""
    src, where = _values_source()
    entries, pos = [], 0
    for so, n, pair in where:
        entries.append((so, n, n, 1, 0, pos, pair))
        pos += -(-(n // ITEM[pair[0]] * ITEM[pair[1]]) // 16) * 16 + 16
    check_cast(ops, device, src, entries, [pos], src_align=src_align)


def _rand(n: int, seed: int = 5) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


# ------------------------------------------------------------------------------------------------
# 2. the alignment grid
# ------------------------------------------------------------------------------------------------
GRID_COUNTS = (1, 3, 4, 7, 8, 9, 17, 50)


def grid_layout(pair):
    """One single-run entry per (dst & 15, src & 15, element count), all in one buffer, one or two
    canary elements between neighbouring outputs, in the greedy order of scatter_model.grid_layout.
    Returns (entries, src_len, buf_len)."""
    si, di = ITEM[pair[0]], ITEM[pair[1]]
    left = {da: [(sa, n) for n in GRID_COUNTS for sa in range(16)] for da in range(0, 16, di)}
    entries, pos, spos = [], 0, 0
    while any(left.values()):
        g = max((di, 2 * di), key=lambda g: len(left[(pos + g) & 15]))
        assert left[(pos + g) & 15], "the greedy order ran dry"
        pos += g
        sa, n = left[pos & 15].pop()
        spos += (sa - spos) & 15
        entries.append((spos, n * si, n * si, 1, 0, pos, pair))
        pos += n * di
        spos += n * si
    return entries, spos, pos + 2 * di


def case_alignment_grid(ops, device, pair) -> None:
    entries, src_len, buf_len = grid_layout(pair)
    si, di = ITEM[pair[0]], ITEM[pair[1]]
    seen = {(off & 15, so & 15, rb // si) for so, rb, _, _, _, off, _ in entries}
    assert len(entries) == (16 // di) * 16 * len(GRID_COUNTS) == len(seen) and 256 < len(entries) <= 1024
    ends = sorted((off, off + rb // si * di) for _, rb, _, _, _, off, _ in entries)
    assert all(b[0] - a[1] in (di, 2 * di) for a, b in zip(ends, ends[1:]))
    check_cast(ops, device, _rand(src_len), entries, [buf_len])


# ------------------------------------------------------------------------------------------------
# 3. the run grid
# ------------------------------------------------------------------------------------------------
RUN_ELEMS = (1, 3, 8, 513, 4097)


def run_grid(pair, stride: str, start: int):
    """RUN_ELEMS x shard_model.N_RUNS with stride `stride` (plus1: every second run's elements sit at
    odd addresses); sources 3 bytes apart; the first output at `start` & 15, the next ones one element
    after their predecessor.  Returns (entries, src_len, buf_len)."""
    si, di = ITEM[pair[0]], ITEM[pair[1]]
    specs = [(ne * si, nr, M.STRIDES[stride](ne * si)) for ne in RUN_ELEMS for nr in M.N_RUNS]
    laid, src_len, _ = M.lay_out(specs)
    entries, pos = [], start
    for so, rb, st, nr, _ in laid:
        entries.append((so, rb, st, nr, 0, pos, pair))
        pos += rb * nr // si * di + di
    return entries, src_len, pos + 16


def case_run_grid(ops, device, pair, stride: str):
    """Every destination alignment of the first output; returns check_cast's buffers per start."""
    out = []
    for start in range(0, 16, ITEM[pair[1]]):
        entries, src_len, buf_len = run_grid(pair, stride, start)
        out += check_cast(ops, device, _rand(src_len, 3), entries, [buf_len], src_align=5)
    return out


# ------------------------------------------------------------------------------------------------
# 4. mixed kinds in one table
# ------------------------------------------------------------------------------------------------
MIXED = ((5, ("F32", "BF16")), (3, ("BF16", "F32")), (1, ("F16", "BF16")), (2, ("F16", "F32")), (7, ("BF16", "F16")),
         (1, ("BF16", "F32")), (3, ("F32", "F16")))


def case_mixed_small(ops, device, gap: int) -> None:
    """Seven small entries of alternating kinds, `gap` bytes (0 or one 2-byte element) apart where the
    next output's item size allows it (a 4-byte output moves up to its next multiple of 4)."""
    entries, pos, spos = [], 6, 1
    for n, pair in MIXED:
        pos += gap
        pos += -pos % ITEM[pair[1]]
        entries.append((spos, n * ITEM[pair[0]], n * ITEM[pair[0]], 1, 0, pos, pair))
        pos += n * ITEM[pair[1]]
        spos += n * ITEM[pair[0]] + 3
    blocks = [{off >> 4, (off + rb // ITEM[p[0]] * ITEM[p[1]] - 1) >> 4} for _, rb, _, _, _, off, p in entries]
    assert sum(bool(a & b) for a, b in zip(blocks, blocks[1:])) >= 3  # neighbours share 16-byte blocks
    check_cast(ops, device, _rand(spos, 9), entries, [pos + 20])


def case_tiles(ops, device) -> None:
    """An F32 -> BF16 entry over more than three tiles of 16 KiB output at dst & 15 = 10, as twelve runs
    of 2049 elements with stride run + 1, next to a BF16 -> F32 entry of three tiles and one element."""
    ne = 12 * 2049
    assert 3 * TILE < 2 * ne < 4 * TILE
    one = 3 * TILE // 4 + 1
    s2 = 11 * (4 * 2049 + 1) + 4 * 2049 + 7
    entries = [(3, 4 * 2049, 4 * 2049 + 1, 12, 0, 10, ("F32", "BF16")), (s2, 2 * one, 2 * one, 1, 1, 16 + 4, ("BF16", "F32"))]
    check_cast(ops, device, _rand(s2 + 2 * one, 17), entries, [10 + 2 * ne + 40, 16 + 4 + 4 * one + 4], src_align=2)


def case_many_small(ops, device) -> None:
    """300 entries of 3 elements inside one tile, kinds in rotation: more than the LDS cache holds."""
    entries, pos, spos = [], 4, 0
    for i in range(300):
        pair = PAIRS[i % len(PAIRS)]
        pos += -pos % ITEM[pair[1]]
        entries.append((spos, 3 * ITEM[pair[0]], 3 * ITEM[pair[0]], 1, 0, pos, pair))
        pos += 3 * ITEM[pair[1]]
        spos += 3 * ITEM[pair[0]] + 1
    assert pos < TILE
    check_cast(ops, device, _rand(spos, 23), entries, [pos + 30])


# ------------------------------------------------------------------------------------------------
# 5. several allocations, descending table
# ------------------------------------------------------------------------------------------------
def case_three_allocations(ops, device) -> None:
    """Entries that end exactly with their buffer's logical range, in ascending and then in descending
    address order (the allocator decides the buffers' own order; the sort is on addresses)."""
    lens = [4096 + 14, 700, 100_004]
    f2b, b2f, h2b = ("F32", "BF16"), ("BF16", "F32"), ("F16", "BF16")
    entries = [(0, 1000, 1000, 1, 0, 18, f2b), (1001, 36, 65, 9, 0, lens[0] - 36 * 9, h2b),  # ends with buffer 0
               (2001, 350, 350, 1, 1, 0, b2f),                                              # a whole buffer
               (3001, 4 * 1025, 4 * 1025 + 1, 12, 2, 2, f2b), (60_001, 50_000, 50_000, 1, 2, 50_004, f2b),
               (120_001, 2 * 6250, 2 * 6250, 1, 2, 75_004, b2f)]                            # ends with buffer 2
    assert 2 * 350 == lens[1] and entries[4][5] + 25_000 == entries[5][5] and 75_004 + 4 * 6250 == lens[2]
    src = _rand(120_001 + 12_500, 29)
    check_cast(ops, device, src, entries, lens, src_align=7)  # ascending within each buffer
    check_cast(ops, device, src, entries, lens, src_align=7, order="descending")


# ------------------------------------------------------------------------------------------------
# 6. nothing to do, refusals
# ------------------------------------------------------------------------------------------------
def case_nothing_to_do(ops, device) -> None:
    p = ("F32", "BF16")
    check_cast(ops, device, _rand(10), [], [64])
    check_cast(ops, device, _rand(10), [(0, 0, 0, 0, 0, 0, p), (10, 0, 4, 3, 0, 16, ("BF16", "F32")), (3, 4, 5, 0, 0, 63, p)],
               [64])


def case_refusals(ops, device, pytest) -> None:
    """Every refusal of ops.slice_scatter_cast names the entry and comes before any launch: the buffers
    keep every canary byte."""
    import torch

    hold, src = place_source(_rand(100), device)
    a = torch.from_numpy(canary(64)).to(device)
    b = torch.from_numpy(canary(64, 1000)).to(device)
    A, B = a.data_ptr(), b.data_ptr()
    K = ops.CAST_KINDS
    f2b, b2f, h2b = K[("F32", "BF16")], K[("BF16", "F32")], K[("F16", "BF16")]
    tab = lambda *e: np.array(list(e), dtype=ops.CAST_DTYPE)

    def run(*entries, buffers=(a, b)):
        ops.slice_scatter_cast(src, tab(*entries), list(buffers))

    with pytest.raises(ValueError, match="entry 1.*unknown kind"):
        run((0, 8, 8, 1, A, f2b), (0, 8, 8, 1, B, len(K)))
    with pytest.raises(ValueError, match="entry 0.*run_bytes 6.*source item"):
        run((0, 6, 6, 2, A, f2b))
    with pytest.raises(ValueError, match="entry 1.*run_bytes 3.*source item"):
        run((0, 8, 8, 1, A, f2b), (0, 3, 4, 2, B, h2b))
    with pytest.raises(ValueError, match="entry 0.*dst_addr.*destination item"):
        run((0, 8, 8, 1, A + 1, f2b))
    with pytest.raises(ValueError, match="entry 1.*dst_addr.*destination item"):
        run((0, 8, 8, 1, A, f2b), (0, 8, 8, 1, B + 2, b2f))
    with pytest.raises(ValueError, match="entry 1.*past the source"):
        run((0, 12, 12, 1, A, f2b), (92, 12, 12, 1, B, f2b))
    with pytest.raises(ValueError, match="entry 0.*past the source"):
        run((0, 4, 49, 3, A, f2b))  # the last run ends at 102
    with pytest.raises(ValueError, match="entry 0.*past the source"):
        run((1 << 63, 2, 1 << 63, 3, A, h2b))  # would wrap around 64 bits
    with pytest.raises(ValueError, match="entry 0.*src_stride"):
        run((0, 4, 3, 2, A, f2b))
    with pytest.raises(ValueError, match="entry 1.*inside one buffer"):
        run((0, 8, 8, 1, A, f2b), (0, 12, 12, 1, B + 44, b2f))  # 24 output bytes: past b's logical end
    with pytest.raises(ValueError, match="entry 0.*inside one buffer"):
        run((0, 12, 12, 1, min(A, B) - 4, f2b))  # starts before the first buffer
    with pytest.raises(ValueError, match="entry 0.*inside one buffer"):
        run((0, 12, 12, 1, A, f2b), buffers=(b,))  # nobody vouches for a
    with pytest.raises(ValueError, match="entry 0.*inside one buffer"):
        run((0, 12, 12, 1, A, f2b), buffers=())
    with pytest.raises(ValueError, match="entry 1.*overlaps entry 0"):
        run((0, 10, 10, 1, A, b2f), (20, 4, 4, 1, A + 18, f2b))  # 20 output bytes: entry 0 ends at A + 20
    with pytest.raises(ValueError, match="entry 2.*overlaps entry 0"):
        run((0, 4, 4, 1, A + 30, f2b), (0, 4, 4, 1, B, f2b), (0, 4, 4, 4, A + 24, f2b))  # its last element is entry 0's
    with pytest.raises(ValueError, match="entry 1.*overlaps the source"):
        run((0, 4, 4, 1, A, f2b), (0, 4, 4, 1, src.data_ptr() + 96, f2b), buffers=(a, hold))
    many = np.broadcast_to(tab((0, 4, 4, 1, A, f2b)), (1 << 32,))  # 2^32 entries without their memory
    with pytest.raises(ValueError, match="4294967296 entries"):
        ops.slice_scatter_cast(src, many, [a, b])
    with pytest.raises(ValueError, match="uint8"):
        ops.slice_scatter_cast(src.view(torch.int16), tab(), [a])
    with pytest.raises(ValueError, match="buffer 1 is on"):
        ops.slice_scatter_cast(src, tab(), [a, torch.empty(4, dtype=torch.uint8, device="meta")])
    assert np.array_equal(a.cpu().numpy(), canary(64)) and np.array_equal(b.cpu().numpy(), canary(64, 1000))
    # all legal: an output that fits only after the conversion halves it, to the last byte of a
    raw = src.cpu().numpy().tobytes()
    run((60, 40, 40, 1, A + 44, f2b), (1, 2, 48, 3, B + 4, b2f), (100, 0, 0, 0, 1, f2b))
    for got, (so, rb, st, nr), pair in ((a.cpu().numpy()[44:], (60, 40, 40, 1), ("F32", "BF16")),
                                        (b.cpu().numpy()[4:16], (1, 2, 48, 3), ("BF16", "F32"))):
        want, nans = _entry(raw, so, rb, st, nr, pair)
        keep = np.repeat(~nans, ITEM[pair[1]])
        assert np.array_equal(got[keep], np.frombuffer(want, dtype=np.uint8)[keep])
