"""GPU: the set-up kernels against the models of setup_models.py: raw xorb packing (k_pack, K7),
the synthetic content generator (k_fill) and the info-hash batch (k_sha1_info_hash, K6); and the
single-buffer CDC scan (k_cdc_candidates, K5) against the host's byte-by-byte scan at the sizes around
its window, step and lane edges.  Destinations are canary-filled and compared in every byte; sources
are checked to be unchanged."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import setup_models as SM
from scatter_model import canary, place_source
from zest_amd import ops, synthetic

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    ops.hip()  # must load: no silent fallback


def _rand(n: int, seed: int) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


def _same(got: np.ndarray, want: np.ndarray, what="") -> None:
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{what}: {bad.size} bytes differ, first at offset {int(bad[0])}"


# ------------------------------------------------------------------------------------------------
# K7: pack_chunks
# ------------------------------------------------------------------------------------------------
PACK_LENS = (0, 1, 2, 3, 4, 5, 7, 8, 63, 64, 65, 255, 256, 257, 259, 8193)


def pack_layout():
    """One chunk per (data_off & 3, (out_off + 8) & 3, len).  The entries stand back to back in `out`,
    0 to 3 canary bytes apart as the wanted misalignment needs; the payloads 0 to 3 bytes apart in
    `data`; the last payload ends with `data`.  -> (data_off, lens, out_off, data_len, out_len)"""
    d_off, lens, o_off, dpos, opos = [], [], [], 0, 8
    for n in PACK_LENS:
        for sa in range(4):
            for da in range(4):
                dpos += (sa - dpos) & 3
                opos += (da - opos) & 3  # out is 16-byte aligned: (out_off + 8) & 3 == out_off & 3
                d_off.append(dpos)
                lens.append(n)
                o_off.append(opos)
                dpos += n
                opos += 8 + n
    return d_off, lens, o_off, dpos, opos + 24


def check_pack(data: np.ndarray, d_off, lens, o_off, out_len: int) -> None:
    hold, d = place_source(data, DEV)
    want = canary(out_len, 9)
    out = torch.from_numpy(want.copy()).to(DEV)
    assert out.data_ptr() % 16 == 0
    ops.pack_chunks(d, np.array(d_off, dtype=np.uint64), np.array(lens, dtype=np.uint32),
                    np.array(o_off, dtype=np.uint64), out)
    SM.pack_model(data, d_off, lens, o_off, want)
    _same(out.cpu().numpy(), want, f"{len(lens)} chunks")
    assert np.array_equal(d.cpu().numpy(), data)


def test_pack_grid_of_misalignments_and_lengths():
    d_off, lens, o_off, data_len, out_len = pack_layout()
    assert len(lens) == 256 and {(d & 3, o & 3, n) for d, n, o in zip(d_off, lens, o_off)} == \
        {(sa, da, n) for sa in range(4) for da in range(4) for n in PACK_LENS}
    gaps = [b - (a + 8 + n) for a, n, b in zip(o_off, lens, o_off[1:])]
    assert set(gaps) == {0, 1, 2, 3}
    assert d_off[-1] + lens[-1] == data_len and lens[-1] == 8193
    data = _rand(data_len, 1)
    check_pack(data, d_off, lens, o_off, out_len)
    for n in (1, 5):  # a launch whose last block has waves without a chunk
        pick = [200 + 3 * i for i in range(n)]
        check_pack(data, [d_off[i] for i in pick], [lens[i] for i in pick], [o_off[i] for i in pick], out_len)


def test_pack_refusals_leave_out_alone():
    hold, d = place_source(_rand(100, 2), DEV)
    out = torch.from_numpy(canary(200, 9)).to(DEV)
    u64, u32 = (lambda *v: np.array(v, dtype=np.uint64)), (lambda *v: np.array(v, dtype=np.uint32))
    with pytest.raises(ValueError, match="out of bounds"):
        ops.pack_chunks(d, u64(0, 91), u32(10, 10), u64(0, 50), out)  # the second payload ends at 101
    with pytest.raises(ValueError, match="out of bounds"):
        ops.pack_chunks(d, u64(0, 10), u32(10, 90), u64(0, 103), out)  # the second entry ends at 201
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), canary(200, 9))
    ops.pack_chunks(d, u64(0, 10), u32(10, 90), u64(0, 102), out)  # to the last byte of both
    want = canary(200, 9)
    SM.pack_model(d.cpu().numpy(), [0, 10], [10, 90], [0, 102], want)
    _same(out.cpu().numpy(), want)


# ------------------------------------------------------------------------------------------------
# k_fill, mode 0: the splitmix64 byte stream
# ------------------------------------------------------------------------------------------------
FILL_OFFS = (0, 1, 7, 8, 9, 12345, 2 ** 32 - 3, 2 ** 40 + 5)
FILL_LENS = (0, 1, 15, 16, 17, 31, 33, 4099)
SLOT = 4160  # a multiple of 16 with room for alignment 15, 4099 bytes and canary on both sides


@pytest.mark.parametrize("seed", [0, 42, 2 ** 64 - 1, -1])
def test_fill_mode0_grid(seed):
    """Destination alignment x stream offset x length, one fill each into a slot of its own of one
    canary buffer.  With destination alignment a the aligned vectors start at stream position
    stream_off + (16 - a) % 16: both the 8-byte-aligned word path and the byte path run, at offsets
    whose word index needs more than 32 bits."""
    cases = [(a, off, n) for a in range(16) for off in FILL_OFFS for n in FILL_LENS]
    want = canary(16 + SLOT * len(cases), 3)
    buf = torch.from_numpy(want.copy()).to(DEV)
    assert buf.data_ptr() % 16 == 0
    fast = 0
    for k, (a, off, n) in enumerate(cases):
        at = 16 + SLOT * k + a
        ops.fill_synthetic(buf[at:at + n], seed, off, 0)
        want[at:at + n] = SM.fill_model(seed, off, n)
        fast += n >= 32 and (off + (16 - a) % 16) % 8 == 0
    assert fast == 32  # per offset two alignments x two lengths take the word path, all others the byte path
    _same(buf.cpu().numpy(), want, f"seed {seed}")


def test_fill_mode0_host_twin_equals_the_device():
    n = 100_000
    host = np.zeros(n, dtype=np.uint8)
    synthetic._host_fill(host, 42, 0)
    for at in (16, 19):  # the word path, and (13 bytes of lead) the byte path
        want = canary(at + n + 32, 4)
        buf = torch.from_numpy(want.copy()).to(DEV)
        ops.fill_synthetic(buf[at:at + n], 42, 0, 0)
        want[at:at + n] = host
        _same(buf.cpu().numpy(), want, f"destination at {at}")
    assert np.array_equal(host, SM.fill_model(42, 0, n))


@pytest.mark.parametrize("stream_off", [5, 0], ids=["word-path", "byte-path"])
def test_fill_mode0_beyond_the_block_cap(stream_off):
    """256 MiB + 64 KiB + 3 bytes at alignment 5: 16,781,311 vectors for the 65,536 x 256 = 16,777,216
    threads of the capped grid, so the first 4095 threads make a second pass.  32 windows of 4 KiB are
    compared: the first, the last with the tail, two across the byte where the second pass begins, 28
    seeded ones; and the canary on both sides."""
    n, a, w = (256 << 20) + (64 << 10) + 3, 5, 4096
    lead = 16 - a
    assert ((n - lead) >> 4) > 65536 * 256 and ((stream_off + lead) % 8 == 0) == (stream_off == 5)
    buf = torch.empty(a + n + 64, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 16 == 0
    edge = torch.from_numpy(canary(a + 64, 6)).to(DEV)
    buf[:a].copy_(edge[:a])
    buf[a + n:].copy_(edge[a:])
    ops.fill_synthetic(buf[a:a + n], 42, stream_off, 0)
    second = lead + 16 * 65536 * 256  # the first byte written in a second pass
    starts = [0, n - w, second - w // 2, second - 16] + \
        [int(x) for x in np.random.default_rng(7).integers(0, n - w, 28)]
    for s in starts:
        got = buf[a + s:a + s + w].cpu().numpy()
        _same(got, SM.fill_model(42, stream_off + s, w), f"window at {s}")
    around = torch.cat([buf[:a], buf[a + n:]]).cpu().numpy()
    assert np.array_equal(around, canary(a + 64, 6))


# ------------------------------------------------------------------------------------------------
# k_fill, mode 1: bf16 ~ N(0, 0.02)
# ------------------------------------------------------------------------------------------------
def _fill1(n: int, seed: int, off: int = 0, align: int = 0) -> np.ndarray:
    """Mode 1 bytes [off, off + n) filled at `align`, canary on both sides checked."""
    want = canary(16 + align + n + 32, 8)
    buf = torch.from_numpy(want.copy()).to(DEV)
    at = 16 + align
    ops.fill_synthetic(buf[at:at + n], seed, off, 1)
    got = buf.cpu().numpy()
    assert np.array_equal(got[:at], want[:at]) and np.array_equal(got[at + n:], want[at + n:])
    return got[at:at + n]


def test_fill_mode1_is_the_same_stream_at_any_alignment_and_offset():
    """Bit-exact against the device itself: a fill at alignment a from an even or odd stream offset
    equals the slice of a fill from offset 0 (an odd offset starts with an element's high byte)."""
    base = _fill1(20_000, 7)
    for a in range(16):
        for off, n in ((0, 100), (1, 100), (2, 33), (7, 4099), (12_344, 1), (12_345, 2), (15_901, 4099)):
            got = _fill1(n, 7, off, a)
            assert np.array_equal(got, base[off:off + n]), (a, off, n)
    far = _fill1(4096, 7, 2 ** 33)  # an element index beyond 32 bits
    assert np.array_equal(_fill1(1001, 7, 2 ** 33 + 1, 3), far[1:1002])
    assert not np.array_equal(far, base[:4096])


@pytest.mark.parametrize("seed", [7, 2 ** 64 - 1])
def test_fill_mode1_against_the_float64_model(seed):
    """2^20 elements.  |gpu - ref| <= 2^-7 |ref| + 0.02 * 2^-10: four bf16 half-ulps, and an absolute
    term for cos near zero.  The bound is loose on purpose (a thousand times below sigma, far above any
    plausible error of the fast log and cos): it catches a wrong element, byte order or scale."""
    count = 1 << 20
    v = SM.bf16_values(_fill1(2 * count, seed))
    assert np.all(np.isfinite(v))
    assert np.all(np.abs(v) <= SM.MODE1_MAX), float(np.abs(v).max())
    ref, bf = SM.fill_model_f64(seed, 0, count)
    excess = np.abs(v - ref) - (2.0 ** -7 * np.abs(ref) + 0.02 * 2.0 ** -10)
    print(f"seed {seed}: max |gpu - ref| {np.abs(v - ref).max():.3e}, largest excess over the bound {excess.max():.3e}, "
          f"patterns equal to the rounded float64 value: {np.mean(SM.bf16_values(bf.view(np.uint8)) == v):.4f}")
    assert excess.max() <= 0, (int(np.argmax(excess)), float(excess.max()))
    assert abs(v.std() - 0.02) < 0.002 and abs(v.mean()) < 0.002


# ------------------------------------------------------------------------------------------------
# K6: sha1_info_hash
# ------------------------------------------------------------------------------------------------
SHA_SIZES = (1, 255, 256, 257, 1000)


@pytest.fixture(scope="module")
def sha_rows():
    """1000 rows: the 256 single-bit rows, all-zero, all-0xFF, random ones; and their digests."""
    rows = _rand(1000 * 32, 3).reshape(1000, 32)
    for i in range(256):
        rows[i] = 0
        rows[i, i >> 3] = 1 << (i & 7)
    rows[256], rows[257] = 0, 0xFF
    return rows, SM.info_hash_model(rows)


@pytest.mark.parametrize("n", SHA_SIZES)
def test_info_hash_all_rows(sha_rows, n):
    rows, want = sha_rows
    for first in (0, 1000 - n):  # the special rows, and random ones
        src = torch.from_numpy(rows[first:first + n].copy()).to(DEV)
        got = ops.sha1_info_hash(src)
        assert got.shape == (n, 20) and got.dtype == torch.uint8
        assert np.array_equal(got.cpu().numpy(), want[first:first + n]), (n, first)
        assert np.array_equal(src.cpu().numpy(), rows[first:first + n])


def test_info_hash_views(sha_rows):
    rows, want = sha_rows
    t = torch.from_numpy(rows.copy()).to(DEV)
    assert np.array_equal(ops.sha1_info_hash(t[::2]).cpu().numpy(), want[::2])  # not contiguous
    assert np.array_equal(ops.sha1_info_hash(t[3:260]).cpu().numpy(), want[3:260])  # a row offset
    wide = torch.from_numpy(_rand(300 * 40, 5).reshape(300, 40)).to(DEV)
    assert np.array_equal(ops.sha1_info_hash(wide[:, 8:]).cpu().numpy(), SM.info_hash_model(wide.cpu().numpy()[:, 8:]))
    assert ops.sha1_info_hash(t[:0]).shape == (0, 20)


@pytest.mark.parametrize("n", SHA_SIZES)
def test_info_hash_stores_nothing_behind_the_last_row(sha_rows, n):
    """Through the binding, into a canary buffer of n * 20 + 32 bytes."""
    rows, want = sha_rows
    hold, src = place_source(rows[:n].reshape(-1), DEV)
    c = canary(16 + 20 * n + 32, 2)
    out = torch.from_numpy(c.copy()).to(DEV)
    ops.hip().sha1_info_hash(src.data_ptr(), n, out.data_ptr() + 16, torch.cuda.current_stream().cuda_stream)
    c[16:16 + 20 * n] = want[:n].reshape(-1)
    _same(out.cpu().numpy(), c, f"n = {n}")
    assert np.array_equal(src.cpu().numpy(), rows[:n].reshape(-1))


# ------------------------------------------------------------------------------------------------
# K5: cdc_candidates on one buffer
# ------------------------------------------------------------------------------------------------
CDC_SIZES = (1, 2, 63, 64, 65, 127, 128, 129, 2032, 2033, 2047, 2048, 2049, 4095, 4097)
DENSE = 0xFF << 56
CDC_SEED = 0  # picked on the CPU: the conditions asserted in test_cdc_small_buffers hold for it


def cdc_cases(seed: int = CDC_SEED):
    """(mask, base misalignment, bytes, the host scan's candidates), fresh random bytes per case."""
    rng = np.random.default_rng(seed)
    grid = [(DENSE, mis) for mis in range(16)] + [(DENSE | 1, mis) for mis in (0, 5, 15)]
    out = []
    for mask, mis in grid:
        for n in CDC_SIZES:
            data = rng.integers(0, 256, n, dtype=np.uint8)
            out.append((mask, mis, data, ops.cdc_candidates(torch.from_numpy(data), mask).tolist()))
    return out


def cdc_cases_tell(cases) -> bool:
    """Candidates inside the first window and step (>= 20 with end offset <= 129 over the grid), and at
    least one in every case that reaches the second lane window at some misalignment (n >= 2033)."""
    early = sum(e <= 129 for _, _, _, want in cases for e in want)
    return early >= 20 and all(want for _, _, data, want in cases if len(data) >= 2033)


def test_cdc_small_buffers():
    """Buffers shorter than the 64-byte window, the 128-byte step and the 2 KiB lane window, and just
    beyond each, at every base misalignment with the dense high-word mask and at three with a mask that
    has a low bit (the full 64-bit compare).  The buffer is a view with other bytes on both sides."""
    cases = cdc_cases()
    assert len(cases) == 19 * len(CDC_SIZES) and cdc_cases_tell(cases)
    for mask, mis, data, want in cases:
        n = len(data)
        around = canary(16 + mis + n + ops.PAD, 1)
        hold = torch.from_numpy(around.copy()).to(DEV)
        view = hold[16 + mis:16 + mis + n]
        view.copy_(torch.from_numpy(data))
        assert view.data_ptr() % 16 == mis
        got = ops.cdc_candidates(view, mask)
        assert got.dtype == np.uint64 and got.tolist() == want, (hex(mask), mis, n)
        around[16 + mis:16 + mis + n] = data
        assert np.array_equal(hold.cpu().numpy(), around)


def test_cdc_capacity_too_small_is_retried():
    data = _rand(10_000, 12)
    want = ops.cdc_candidates(torch.from_numpy(data), DENSE).tolist()
    assert len(want) > 20
    hold = ops.padded_empty(10_000 + 9, DEV)
    hold[9:].copy_(torch.from_numpy(data))
    assert ops.cdc_candidates(hold[9:], DENSE, capacity=3).tolist() == want
    assert ops.cdc_candidates(hold[9:], DENSE).tolist() == want
