"""Executable model of the batched LZ4 decoder's algorithm (csrc/gpu/lz4seq.hip), run on the CPU.

The kernel splits LZ4 into a serial parse (sequences -> 64-record batches) and a lane-parallel
execute: literal bytes, then match bytes, 64 per pass, each match byte reading its periodic
source `start - off + k % off`, with sources written by the same pass chased to the writer's own
source, and near sources (< kRing behind the batch end) read from a per-wave history ring that only
short batches may trust.  This file re-implements exactly those rules with numpy "lanes" and checks
the result against the host LZ4 decoder on frames from the host encoder, so the algorithm (not just
one GPU run) is pinned: every data shape the GPU tests use plus RLE runs, long literal runs, far
repeats and overlapping short offsets.
"""
from __future__ import annotations

import struct

import numpy as np
import pytest

from zest_amd import _core as C

WAVE = 64
RING = 4096


def parse_frame(frame: bytes, stats: dict | None = None):
    """LZ4 frame -> list of (literal_pos, literal_len, match_len, offset) records, literal runs split
    at 0xFFFF and matches at 0x7FFF exactly like the kernel's emit().  stats["split_records"] counts
    the records beyond one per sequence."""
    assert struct.unpack_from("<I", frame, 0)[0] == 0x184D2204
    flg = frame[4]
    ip = 7 + (8 if flg & 8 else 0) + (4 if flg & 1 else 0)
    bck = 4 if flg & 0x10 else 0
    recs = []

    def emit(lp, lit, ml, off):
        n0 = len(recs)
        _emit(lp, lit, ml, off)
        if stats is not None:
            stats["split_records"] = stats.get("split_records", 0) + len(recs) - n0 - 1

    def _emit(lp, lit, ml, off):
        while lit > 0xFFFF:
            recs.append((lp, 0xFFFF, 0, 0))
            lp += 0xFFFF
            lit -= 0xFFFF
        first = True
        while first or ml:
            m = min(ml, 0x7FFF)
            recs.append((lp, lit, m, off if m else 0))
            lp += lit
            lit = 0
            ml -= m
            first = False

    while True:
        bs = struct.unpack_from("<I", frame, ip)[0]
        ip += 4
        if bs == 0:
            break
        ln = bs & 0x7FFFFFFF
        if bs >> 31:
            emit(ip, ln, 0, 0)
            ip += ln
        else:
            bend = ip + ln
            while True:
                tok = frame[ip]
                ip += 1
                lit = tok >> 4
                if lit == 15:
                    while True:
                        b = frame[ip]
                        ip += 1
                        lit += b
                        if b != 255:
                            break
                lp = ip
                ip += lit
                if ip == bend:
                    emit(lp, lit, 0, 0)
                    break
                off = frame[ip] | (frame[ip + 1] << 8)
                ip += 2
                ml = tok & 15
                if ml == 15:
                    while True:
                        b = frame[ip]
                        ip += 1
                        ml += b
                        if b != 255:
                            break
                emit(lp, lit, ml + 4, off)
        ip += bck
    return recs


FLUSH_ABOVE = WAVE - 8  # kFlushAbove: a batch holding more records than this is executed


def kernel_batches(frame: bytes, stats: dict | None = None) -> list[int]:
    """Record counts of the batches the one-wave parse (lz4seq.hip parse_frame) hands to exec_batch,
    in order: its fast loop takes sequences without length bytes that start more than 18 bytes
    before the block end, up to 64 records; the general path takes one sequence of any kind when the
    batch holds at most FLUSH_ABOVE records.  stats["handover"] collects, per hand-over from the
    fast loop to the general path, the distance from the sequence's token to the block end."""
    flg = frame[4]
    ip = 7 + (8 if flg & 8 else 0) + (4 if flg & 1 else 0)
    bck = 4 if flg & 0x10 else 0
    out = []
    n = 0

    def nrec(lit, ml):  # emit()
        c = 0
        while True:
            l = min(lit, 0xFFFF)
            m = 0 if lit > 0xFFFF else min(ml, 0x7FFF)
            c += 1
            lit -= l
            ml -= m
            if not (lit or ml):
                return c

    def chain(v, ip):
        while True:
            b = frame[ip]
            ip += 1
            v += b
            if b != 255:
                return v, ip

    while True:
        if n > FLUSH_ABOVE:
            out.append(n)
            n = 0
        bs = struct.unpack_from("<I", frame, ip)[0]
        ip += 4
        if bs == 0:
            break
        ln = bs & 0x7FFFFFFF
        if bs >> 31:
            n += nrec(ln, 0)
            ip += ln
        else:
            bend = ip + ln
            while True:
                if n > FLUSH_ABOVE:
                    out.append(n)
                    n = 0
                lim = bend - 18 if bend > 18 else 0
                iters = min(WAVE - n, (lim - ip + 16) // 17) if ip < lim else 0
                while iters > 0 and frame[ip] >> 4 != 15 and frame[ip] & 15 != 15:
                    ip += 1 + (frame[ip] >> 4) + 2
                    n += 1
                    iters -= 1
                if n > FLUSH_ABOVE or (iters == 0 and ip < lim):
                    continue
                if stats is not None:
                    stats.setdefault("handover", set()).add(bend - ip)
                tok = frame[ip]
                ip += 1
                lit, ml = tok >> 4, tok & 15
                if lit == 15:
                    lit, ip = chain(lit, ip)
                ip += lit
                if ip == bend:
                    n += nrec(lit, 0)
                    break
                ip += 2
                if ml == 15:
                    ml, ip = chain(ml, ip)
                n += nrec(lit, ml + 4)
        ip += bck
    if n:
        out.append(n)
    return out


def model_decode(frame: bytes, ulen: int, batch=WAVE, stats: dict | None = None) -> bytes:
    """batch: records per batch, or the list of batch sizes (kernel_batches).  stats (optional)
    counts the paths taken: "chase" same-pass chase iterations, "far" / "near" match bytes of short
    batches read from HBM / from the ring, "long_batches", "ring_rebuilds", "wide_runs" (literal
    runs a long batch copies 1 KiB at a time) and "split_records"."""
    recs = parse_frame(frame, stats)

    def count(key, n=1):
        if stats is not None:
            stats[key] = stats.get(key, 0) + int(n)

    out = np.full(ulen, -1, dtype=np.int64)       # HBM (what stores have produced so far)
    ring = np.full(RING, -1, dtype=np.int64)      # the wave's LDS history
    src = np.frombuffer(frame, dtype=np.uint8)
    obase = 0
    sizes = [batch] * ((len(recs) + batch - 1) // batch) if isinstance(batch, int) else list(batch)
    assert sum(sizes) >= len(recs)
    b0 = 0
    for size in sizes:                            # the kernel executes 57..64 records at a time
        batch_recs = recs[b0:b0 + size]
        b0 += size
        lit = np.array([r[1] for r in batch_recs], dtype=np.int64)
        ml = np.array([r[2] for r in batch_recs], dtype=np.int64)
        off = np.array([r[3] for r in batch_recs], dtype=np.int64)
        lpos = np.array([r[0] for r in batch_recs], dtype=np.int64)
        opos = obase + np.cumsum(lit + ml) - lit - ml
        mstart = opos + lit
        span = int((lit + ml).sum())
        oend = obase + span
        # literal phase (byte t of the batch's literal bytes on lane t % 64)
        li = np.cumsum(lit)
        for t in range(int(li[-1]) if len(li) else 0):
            s = int(np.searchsorted(li, t, side="right"))
            k = t - (li[s] - lit[s])
            p = opos[s] + k
            out[p] = ring[p % RING] = src[lpos[s] + k]
        # match passes
        mi = np.cumsum(ml)
        mtot = int(mi[-1]) if len(mi) else 0
        short = span + 4 * WAVE < RING
        if not short:
            count("long_batches")
            count("wide_runs", (lit >= 512).sum())
        for t0 in range(0, mtot, WAVE):
            t = np.arange(t0, min(t0 + WAVE, mtot))
            s = np.searchsorted(mi, t, side="right")
            k = t - (mi[s] - ml[s])
            o = np.maximum(off[s], 1)
            d = mstart[s] + k
            q = mstart[s] - o + k % o
            while True:  # chase sources written by this same pass
                j = np.searchsorted(d, q)
                pend = (j < len(d)) & (d[np.minimum(j, len(d) - 1)] == q)
                if not pend.any():
                    break
                count("chase")
                q = np.where(pend, q[np.minimum(j, len(d) - 1)], q)
            if short:
                far = oend - q >= RING
                count("far", far.sum())
                count("near", (~far).sum())
                v = np.where(far, out[q], ring[q % RING])
            else:
                v = out[q]          # long batch: HBM read-back after s_waitcnt
            assert (v >= 0).all(), "read a byte before it was written"
            out[d] = v
            ring[d % RING] = v
        if not short:               # rebuild the ring from HBM
            count("ring_rebuilds")
            lo = max(0, oend - RING)
            ring[np.arange(lo, oend) % RING] = out[lo:oend]
        obase = oend
    assert obase == ulen and (out >= 0).all()
    return out.astype(np.uint8).tobytes()


def _bf16(n, seed):
    w = np.random.default_rng(seed).standard_normal(n // 2).astype(np.float32) * 0.02
    return (w.view(np.uint32) >> 16).astype(np.uint16).tobytes()


def _cases():
    rng = np.random.default_rng(3)
    phrase = rng.integers(0, 256, 3000, dtype=np.uint8)
    far = np.resize(phrase, 60_000).copy()
    far[rng.integers(0, far.size, 500)] = rng.integers(0, 256, 500, dtype=np.uint8)
    return {
        "bf16": _bf16(65_536, 1),
        "bf16_128k": _bf16(131_072, 2),
        "zeros": bytes(131_072),
        "rle_short_offsets": (b"ab" * 9000 + b"xyz" * 7000 + b"q" * 20_000),
        "long_literals_then_repeats": rng.integers(0, 256, 40_000, dtype=np.uint8).tobytes() + b"hello " * 4000,
        "lowent": (rng.integers(0, 8, 65_536, dtype=np.uint8) * 31).tobytes(),
        "far_repeats": far.tobytes(),
        "text": b"zest xorb ingest test line. " * 2500,
        "sparse": np.where(rng.random(65_536) < 0.02, rng.integers(0, 256, 65_536), 0).astype(np.uint8).tobytes(),
    }


@pytest.mark.parametrize("policy", ["lz4", "bg4"])
@pytest.mark.parametrize("name", sorted(_cases()))
def test_batched_decode_model_matches_host_decoder(name, policy):
    data = _cases()[name]
    scheme, frame = C.compress_chunk(data, policy)
    if scheme == 0:
        pytest.skip("stored uncompressed")
    grouped = C.decompress_chunk(1, frame, len(data))  # the LZ4 stream's own output (BG4: grouped)
    for batch in (64, 59, 37):
        assert model_decode(frame, len(data), batch) == grouped, batch
    assert C.decompress_chunk(scheme, frame, len(data)) == data
