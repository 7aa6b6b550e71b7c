"""GPU: the serve-pack kernel (csrc/gpu/serve.hip, ops.serve_pack) against the plain-Python model,
byte-exact.  Every call writes into its own slot of one 0xA5-filled buffer, so one comparison checks
the served bytes and the 64-byte canaries before and after every window."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import serve_pack_model as M
from zest_amd import ops

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
CANARY = 64


def _run(arena, offs, lens, base=None, shift=0):
    """Upload a family's arena to a 16-byte aligned device address (+ shift) -> (run, serialized)."""
    buf = ops.padded_empty(len(arena) + 16, DEV) if base is None else base
    assert buf.data_ptr() % 16 == 0
    buf[shift:shift + len(arena)].copy_(torch.from_numpy(arena))
    addrs = np.uint64(buf.data_ptr() + shift) + np.asarray(offs, dtype=np.uint64)
    run = ops.ServeRun(addrs, lens, buffers=[buf])
    return run, M.serialize(M.chunks_of(arena, offs, lens))


def _check_windows(run, ser, windows):
    """Serve every (lo, hi) window into its own canaried slot; compare the whole buffer once."""
    ser = np.frombuffer(ser, dtype=np.uint8)
    slots, at = [], 0
    for lo, hi in windows:
        slots.append(at + CANARY)
        at += 2 * CANARY + (hi - lo + 15) // 16 * 16
    big = torch.full((at,), 0xA5, dtype=torch.uint8, device=DEV)
    want = np.full(at, 0xA5, dtype=np.uint8)
    for (lo, hi), o in zip(windows, slots):
        ops.serve_pack(run, lo=lo, hi=hi, out=big[o:o + hi - lo])
        want[o:o + hi - lo] = ser[lo:hi]
    got = big.cpu().numpy()
    if not np.array_equal(got, want):
        bad = int(np.flatnonzero(got != want)[0])
        k = int(np.searchsorted(slots, bad, side="right")) - 1
        raise AssertionError(f"byte {bad} differs: window {windows[max(k, 0)]} slot at {slots[max(k, 0)]}")


def _pieces(total, step):
    return [(a, min(total, a + step)) for a in range(0, total, step)]


@pytest.fixture(scope="module")
def edges():
    arena, offs, lens = M.family_edges()
    run, ser = _run(arena, offs, lens)
    return run, ser, M.ser_ends(M.chunks_of(arena, offs, lens))


def test_tiny_chunks_whole_stream():
    run, ser = _run(*M.family_tiny())
    _check_windows(run, ser, [(0, len(ser))])
    assert ops.serve_pack(run).cpu().numpy().tobytes() == ser


def test_tiny_chunks_every_window_of_first_256_bytes():
    run, ser = _run(*M.family_tiny())
    _check_windows(run, ser, [(lo, hi) for lo in range(257) for hi in range(lo, 257)])


def test_source_alignment():
    arena, offs, lens = M.family_alignment()
    run, ser = _run(arena, offs, lens)
    assert sorted(int(a) % 16 for a in run.src[:16]) == list(range(16)) and run.src[16] == run.src[17] == run.src[3]
    _check_windows(run, ser, [(0, len(ser))] + _pieces(len(ser), 4104) + _pieces(len(ser), 1000))


def test_edges_whole_run(edges):
    run, ser, _ = edges
    _check_windows(run, ser, [(0, len(ser))])


@pytest.mark.parametrize("piece", [16, 48, 4096, 1 << 20])
def test_edges_in_pieces(edges, piece):
    run, ser, ends = edges
    if piece < 4096:
        # 16- and 48-byte pieces over all 4 MiB would be 275k / 92k launches (seconds).  They run
        # back to back over the whole first chunk, 512 bytes around both ends of the exact-size
        # chunks (65536, 65537, 131072) and the stream's last KiB; the 4 KiB and 1 MiB pieces
        # cover every byte of the run.
        spans = [(0, ends[0] + 264)] + [(ends[k] - 251, ends[k] + 261) for k in (4, 5, 6, 39, 40)]
        spans.append((len(ser) - 1021, len(ser)))
        wins = [(a + x, min(b, a + x + piece)) for a, b in spans for x in range(0, b - a, piece)]
    else:
        wins = _pieces(len(ser), piece)
    _check_windows(run, ser, wins)
    if piece >= 4096:  # concatenated pieces are the stream
        out = torch.empty(len(ser), dtype=torch.uint8, device=DEV)
        for lo, hi in wins:
            ops.serve_pack(run, lo=lo, hi=hi, out=out[lo:hi])
        assert out.cpu().numpy().tobytes() == ser


def test_edges_windows_around_every_boundary(edges):
    run, ser, ends = edges
    _check_windows(run, ser, M.boundary_windows(ends, len(ser)))


def test_table_pressure():
    run, ser = _run(*M.family_table())
    _check_windows(run, ser, [(0, len(ser)), (5, len(ser) - 3)] + _pieces(len(ser), 16384 + 48))


def test_destination_in_pinned_host_memory(edges):
    run, ser, _ = edges
    H = ops.hip()
    cap = len(ser) + 2 * CANARY
    p = H.host_malloc(cap)
    try:
        import ctypes

        host = np.ctypeslib.as_array((ctypes.c_uint8 * cap).from_address(p))
        for wins in ([(0, len(ser))], _pieces(len(ser), 1 << 20), _pieces(len(ser), 4096)):
            host[:] = 0xA5
            for lo, hi in wins:
                assert ops.serve_pack(run, lo=lo, hi=hi, out=(p + CANARY + lo, hi - lo)) is None
            torch.cuda.current_stream(DEV).synchronize()
            assert host[CANARY:CANARY + len(ser)].tobytes() == ser
            assert (host[:CANARY] == 0xA5).all() and (host[CANARY + len(ser):] == 0xA5).all()
    finally:
        torch.cuda.synchronize(DEV)
        H.host_free(p)
    # a pinned torch tensor as `out`
    t = torch.full((70000 + 2 * CANARY,), 0xA5, dtype=torch.uint8).pin_memory()
    got = ops.serve_pack(run, lo=5, hi=70005, out=t[CANARY:CANARY + 70000])
    torch.cuda.current_stream(DEV).synchronize()
    assert got.numpy().tobytes() == ser[5:70005]
    assert t[:CANARY].eq(0xA5).all() and t[CANARY + 70000:].eq(0xA5).all()


@pytest.mark.parametrize("where", ["start", "end"])
def test_source_at_buffer_start_and_end(where):
    rng = np.random.default_rng(9)
    n = 3 * 4096 + 5
    data = rng.integers(0, 256, n, dtype=np.uint8)
    buf = ops.padded_empty(n, DEV)
    buf.copy_(torch.from_numpy(data))
    lens = [4096, 4101, 4096] if where == "start" else [4096, 4096, 4101]
    offs = np.cumsum(lens) - lens  # first chunk at byte 0, last chunk ends at the buffer's last byte
    assert offs[-1] + lens[-1] == n
    run = ops.ServeRun(np.uint64(buf.data_ptr()) + offs.astype(np.uint64), lens, buffers=[buf])
    ser = M.serialize(M.chunks_of(data, offs, lens))
    _check_windows(run, ser, [(0, len(ser)), (0, 31), (len(ser) - 31, len(ser)), (8, len(ser) - 1)])


def test_rejects_bad_descriptors():
    buf = ops.padded_empty(4096, DEV)
    with pytest.raises(ValueError):
        ops.ServeRun([buf.data_ptr() + 4000], [97], buffers=[buf])
    run = ops.ServeRun([buf.data_ptr()], [100], buffers=[buf])
    with pytest.raises(ValueError):
        ops.serve_pack(run, lo=0, hi=109)
    with pytest.raises(ValueError):
        ops.serve_pack(run, out=torch.empty(200, dtype=torch.uint8, device=DEV)[8:])
